"""The reference's optimizer on the HIP path: ``torch.optim.Adam(l, lr=0.0, eps=1e-15)`` of ``training_setup``
(``scene/gaussian_model.py:240-268``), stepped at ``train.py:136-139``, and its learning-rate schedule
(``utils/general_utils.py:29-62``, ``scene/gaussian_model.py:271-277``).

``Adam`` is a drop-in for ``torch.optim.Adam`` whose ``step()`` is one launch of ``csrc/adam.hip`` per 16 tensors
(``gsr_adam_step``) instead of torch's ~8 ``_foreach_*`` passes.  It gives the bits of torch's default (``foreach``)
path for float32 and keeps torch's state layout -- ``{"step": float32 CPU tensor, "exp_avg", "exp_avg_sq"}`` per
parameter -- so the code that edits ``optimizer.state`` (``densify.densify_and_prune``, ``layout.reorder_gaussians_``,
the reference's ``replace_tensor_to_optimizer`` / ``_prune_optimizer``) and ``state_dict()`` work unchanged, in both
directions.  It covers what the reference uses: no weight decay, amsgrad, maximize, capturable, differentiable or fused
variants (``ValueError``), and float32 contiguous parameters on a ROCm GPU (no CPU path).

``SparseGaussianAdam`` is ``Adam`` with a row mask: ``step(visibility)`` updates the Gaussians a frame saw and leaves the
rest of the model's memory alone (``gsr_adam_step_rows``); ``OptimizationParams.optimizer_type = "sparse_adam"``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib
from .densify import FORK_ATTR, FORK_FLAG, GROUP_ATTR

_UNSUPPORTED = ("weight_decay", "amsgrad", "maximize", "capturable", "differentiable", "fused", "decoupled_weight_decay")


def _scalar_dtype():
    # torch.optim.optimizer._get_scalar_dtype(): the dtype of torch's CPU "step" tensors
    return torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32


def _check_group(group) -> None:
    for key in _UNSUPPORTED:
        if group.get(key):
            raise ValueError(f"mvs_gaussian_splatting_amd.optim.Adam does not support {key}={group[key]!r} "
                             "(the reference's Adam uses none of them)")


def adam_scalars(lr: float, betas: Tuple[float, float], eps: float, step: float) -> Dict[str, float]:
    """The per-tensor scalars of one step as ``_multi_tensor_adam`` computes them (in double, ``step`` the count after
    its increment); ``gsr_adam_step`` receives each converted to float, where torch's foreach kernels convert them."""
    beta1, beta2 = betas
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return {"lerp_weight": 1 - beta1, "beta2": beta2, "sq_weight": 1 - beta2, "bc2_sqrt": bias_correction2 ** 0.5,
            "eps": eps, "step_size": (lr / bias_correction1) * -1}


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam`` with the update of ``csrc/adam.hip``: same signature, state and results (bit for bit
    against torch's default ``foreach`` step on float32).  ``foreach`` is accepted and ignored."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if isinstance(lr, torch.Tensor):
            if lr.numel() != 1:
                raise ValueError("Tensor lr must be 1-element")
            lr = lr.item()
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        betas = tuple(float(b) for b in betas)
        defaults = {"lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay, "amsgrad": amsgrad,
                    "maximize": maximize, "foreach": foreach, "capturable": capturable,
                    "differentiable": differentiable, "fused": fused, "decoupled_weight_decay": decoupled_weight_decay}
        _check_group(defaults)
        super().__init__(params, defaults)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            for key, default in (("weight_decay", 0), ("amsgrad", False), ("maximize", False), ("foreach", None),
                                 ("capturable", False), ("differentiable", False), ("fused", None),
                                 ("decoupled_weight_decay", False)):
                group.setdefault(key, default)

    def _checked(self) -> List[Tuple]:
        """``(param, lr, betas, eps, group name)`` of every parameter that has a gradient; every check of ``step``, and
        no change to any state."""
        todo = []
        for group in self.param_groups:
            _check_group(group)
            lr = group["lr"]
            lr = lr.item() if isinstance(lr, torch.Tensor) else float(lr)
            betas = tuple(b.item() if isinstance(b, torch.Tensor) else float(b) for b in group["betas"])
            eps = float(group["eps"])
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise _lib.GsrError("Adam.step needs ROCm GPU parameters (no CPU path)")
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                    raise TypeError(f"Adam.step supports float32 parameters and gradients, got {p.dtype} / "
                                    f"{p.grad.dtype}")
                if p.is_sparse or p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients")
                if not p.is_contiguous():
                    raise ValueError("Adam.step needs contiguous parameters")
                for name in ("exp_avg", "exp_avg_sq"):
                    t = self.state[p].get(name) if p in self.state else None
                    if t is not None and (t.device != p.device or t.dtype != torch.float32 or t.numel() != p.numel()
                                          or not t.is_contiguous()):
                        raise ValueError(f"state[{name!r}] must be a contiguous float32 tensor like its parameter")
                todo.append((p, lr, betas, eps, group.get("name")))
        return todo

    def _advance(self, todo) -> List[Tuple]:
        """Creates the missing states, counts the step of every entry of ``todo`` and returns, per entry,
        ``(param, grad, exp_avg, exp_avg_sq, scalars of that count)``."""
        items = []
        for p, lr, betas, eps, _ in todo:
            grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            state = self.state[p]
            if len(state) == 0:                                      # torch's _init_group, capturable = fused = False
                state["step"] = torch.tensor(0.0, dtype=_scalar_dtype())
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["step"] += 1
            items.append((p, grad, state["exp_avg"], state["exp_avg_sq"],
                          adam_scalars(lr, betas, eps, state["step"].item())))
        return items

    @staticmethod
    def _launch(items, visibility=None) -> None:
        """``gsr_adam_step`` over ``items`` (``gsr_adam_step_rows`` with a ``visibility``), 16 tensors a launch, on the
        current stream of each parameter's device."""
        per_device: Dict[torch.device, List[Tuple]] = {}
        for item in items:
            per_device.setdefault(item[0].device, []).append(item)
        lib = _lib.load() if per_device else None
        for dev, group in per_device.items():
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                for first in range(0, len(group), _lib.ADAM_MAX_TENSORS):
                    chunk = group[first:first + _lib.ADAM_MAX_TENSORS]
                    batch = _lib.GsrAdamBatch() if visibility is None else _lib.GsrAdamRowsBatch()
                    batch.count = len(chunk)
                    for e, (p, g, m, v, sc) in zip(batch.t, chunk):
                        e.param, e.grad, e.exp_avg, e.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
                        e.numel = p.numel()
                        for k, val in sc.items():
                            setattr(e, k, val)
                    if visibility is None:
                        _lib.check(lib.gsr_adam_step(C.byref(batch), stream), "gsr_adam_step")
                    else:
                        batch.visibility, batch.rows = visibility.data_ptr(), visibility.numel()
                        batch.visibility_kind = _lib.ADAM_VIS_I32 if visibility.dtype == torch.int32 else _lib.ADAM_VIS_U8
                        _lib.check(lib.gsr_adam_step_rows(C.byref(batch), stream), "gsr_adam_step_rows")

    @torch.no_grad()
    def step(self, closure=None):
        """One Adam step of every parameter whose ``.grad`` is not None (the others keep their step count and
        moments), enqueued on the current stream of the parameters' device; no host synchronisation."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        todo = self._checked()                                       # every check before any state changes
        self._launch(self._advance(todo))
        return loss


class SparseGaussianAdam(Adam):
    """``Adam`` that can step only the rows -- the Gaussians -- one frame saw (``gsr_adam_step_rows``): the rows of
    every other Gaussian are neither read nor written, which is where the time of a step goes.  Same constructor, same
    state (``step`` float32 CPU tensor, ``exp_avg``, ``exp_avg_sq``), so ``state_dict()`` moves freely between this
    class, ``Adam`` and ``torch.optim.Adam``, and the code that edits ``optimizer.state`` works unchanged.

    After ``step(visibility)`` the visible rows hold what the dense step would have produced from the same state, bit
    for bit, and every other row is untouched: its moments do not decay and its gradient is never read.  ``step``
    counts once per call for every stepped parameter, seen rows or not, and the scalars are ``adam_scalars`` of that
    count.  This is deliberately not the sparse Adam kernel of upstream Inria 3DGS, which drops the bias correction:
    keeping torch's scalars keeps checkpoints interchangeable and the result checkable against ``torch.optim.Adam``."""

    @torch.no_grad()
    def step(self, visibility=None, dense=(), closure=None):
        """visibility: None -- exactly ``Adam.step()`` -- or a contiguous device tensor ``[P]``, bool / uint8 (visible
        iff non-zero) or int32 (visible iff > 0: ``radii`` as the rasterizer returns it).  Every parameter that has a
        gradient must have ``shape[0] == P`` (``ValueError`` before any state changes); parameters without one are
        skipped unchecked, as on the iteration after a densification.
        dense: names of parameter groups that take the dense update in the same step."""
        if visibility is None:
            return super().step(closure)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not isinstance(visibility, torch.Tensor) or visibility.dtype not in (torch.bool, torch.uint8, torch.int32):
            raise TypeError("visibility must be a bool, uint8 or int32 tensor, got "
                            f"{visibility.dtype if isinstance(visibility, torch.Tensor) else type(visibility).__name__}")
        if visibility.dim() != 1 or not visibility.is_contiguous():
            raise ValueError(f"visibility must be a contiguous [P] tensor, got shape {tuple(visibility.shape)}")
        dense = (dense,) if isinstance(dense, str) else tuple(dense)
        P = visibility.shape[0]
        for group in self.param_groups:
            if group.get("name") in dense:
                continue
            for p in group["params"]:
                if p.grad is not None and (p.dim() == 0 or p.shape[0] != P):
                    raise ValueError(f"visibility has {P} rows, a parameter of group {group.get('name')!r} has shape "
                                     f"{tuple(p.shape)}")
        todo = self._checked()
        for p, *_ in todo:
            if visibility.device != p.device:
                raise ValueError(f"visibility is on {visibility.device}, a parameter on {p.device}")
        items = self._advance(todo)
        is_dense = [name in dense for *_, name in todo]
        self._launch([it for it, d in zip(items, is_dense) if d])
        self._launch([it for it, d in zip(items, is_dense) if not d], visibility)
        return loss


def expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """``get_expon_lr_func`` (``utils/general_utils.py:29-62``): log-linear decay from ``lr_init`` at step 0 to
    ``lr_final`` at ``max_steps``, eased in over ``lr_delay_steps`` from ``lr_init * lr_delay_mult``."""
    def helper(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        if lr_delay_steps > 0:
            delay_rate = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
        else:
            delay_rate = 1.0
        t = np.clip(step / max_steps, 0, 1)
        log_lerp = np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)
        return delay_rate * log_lerp
    return helper


def param_groups(model, opt) -> List[dict]:
    """The group list ``l`` of ``training_setup`` (``:244-262``): the six plain groups, then the fork's groups whose
    model flags are set (``densify.FORK_FLAG``), in the reference's order."""
    lrs = {"xyz": opt.position_lr_init * model.spatial_lr_scale, "f_dc": opt.feature_lr,
           "f_rest": opt.feature_lr / 20.0, "opacity": opt.opacity_lr, "scaling": opt.scaling_lr,
           "rotation": opt.rotation_lr}
    fork_lr = {"dirs_prob": "growdirs_lr", "conti_dirs": "growdirs_lr", "grow_dist": "growdistance_lr",
               "split_distance": "splitdistance_lr", "split_scale": "splitscale_lr"}
    groups = [{"params": [getattr(model, a)], "lr": lrs[k], "name": k} for k, a in GROUP_ATTR.items()]
    for k, a in FORK_ATTR.items():
        if getattr(model, FORK_FLAG[k], False):
            groups.append({"params": [getattr(model, a)], "lr": getattr(opt, fork_lr[k]), "name": k})
    return groups


OPTIMIZER_TYPES = {"default": Adam, "sparse_adam": SparseGaussianAdam}


def optimizer_class(opt):
    """The class ``opt.optimizer_type`` names (``"default"`` where ``opt`` has no such field): ``Adam`` or
    ``SparseGaussianAdam``; ``ValueError`` for anything else."""
    kind = getattr(opt, "optimizer_type", "default")
    if kind not in OPTIMIZER_TYPES:
        raise ValueError(f"optimizer_type must be one of {sorted(OPTIMIZER_TYPES)}, got {kind!r}")
    return OPTIMIZER_TYPES[kind]


EXPOSURE_LR_INIT, EXPOSURE_LR_FINAL = 0.01, 0.001      # upstream's defaults, for an `opt` without the fields


def training_setup(model, opt, optimizer_cls=None):
    """``GaussianModel.training_setup(training_args)`` (``scene/gaussian_model.py:240-268``) with this module's
    ``Adam``: sets ``percent_dense``, zeroed ``xyz_gradient_accum`` / ``denom`` ``[P, 1]`` on the model's device
    (and ``xyz_gradient_accum_abs`` with ``opt.abs_grad``, else None),
    ``optimizer`` (``lr=0.0, eps=1e-15``) and ``xyz_scheduler_args``; for a model with exposures
    (``GaussianModel.setup_exposures``) also ``exposure_optimizer`` (``Adam([_exposure], lr=0.0, eps=1e-8)``, always
    dense) and ``exposure_scheduler_args`` over ``opt.iterations`` steps, else ``exposure_optimizer = None``.  optimizer_cls: None takes the class
    ``opt.optimizer_type`` names (``optimizer_class``).  Returns the optimizer."""
    if optimizer_cls is None:
        optimizer_cls = optimizer_class(opt)
    model.percent_dense = opt.percent_dense
    P, dev = model._xyz.shape[0], model._xyz.device
    model.xyz_gradient_accum = torch.zeros((P, 1), device=dev)
    model.denom = torch.zeros((P, 1), device=dev)
    # the absolute-gradient accumulator of AbsGS / PGSR: only for a run that asked for it (opt.abs_grad)
    model.xyz_gradient_accum_abs = torch.zeros((P, 1), device=dev) if getattr(opt, "abs_grad", False) else None
    model.optimizer = optimizer_cls(param_groups(model, opt), lr=0.0, eps=1e-15)
    model.xyz_scheduler_args = expon_lr_func(lr_init=opt.position_lr_init * model.spatial_lr_scale,
                                             lr_final=opt.position_lr_final * model.spatial_lr_scale,
                                             lr_delay_mult=opt.position_lr_delay_mult,
                                             max_steps=opt.position_lr_max_steps)
    # per-image exposures (upstream 3DGS): an optimizer of their own, only for a model that had setup_exposures()
    model.exposure_optimizer = None
    if getattr(model, "_exposure", None) is not None:
        model.exposure_optimizer = Adam([model._exposure], lr=0.0, eps=1e-8)
        model.exposure_scheduler_args = expon_lr_func(getattr(opt, "exposure_lr_init", EXPOSURE_LR_INIT),
                                                      getattr(opt, "exposure_lr_final", EXPOSURE_LR_FINAL),
                                                      lr_delay_steps=getattr(opt, "exposure_lr_delay_steps", 0),
                                                      lr_delay_mult=getattr(opt, "exposure_lr_delay_mult", 0.0),
                                                      max_steps=opt.iterations)
    return model.optimizer


def update_learning_rate(model, iteration):
    """``GaussianModel.update_learning_rate`` (``:271-277``): the ``xyz`` group's lr from ``xyz_scheduler_args``;
    returns it (None without an ``xyz`` group).  The exposure optimizer's lr follows ``exposure_scheduler_args``."""
    if getattr(model, "exposure_optimizer", None) is not None:
        for group in model.exposure_optimizer.param_groups:
            group["lr"] = model.exposure_scheduler_args(iteration)
    for group in model.optimizer.param_groups:
        if group["name"] == "xyz":
            lr = model.xyz_scheduler_args(iteration)
            group["lr"] = lr
            return lr
    return None


__all__ = ["Adam", "SparseGaussianAdam", "adam_scalars", "expon_lr_func", "optimizer_class", "param_groups",
           "training_setup", "update_learning_rate"]
