"""MCMC densification ("3DGS as Markov-chain Monte Carlo") on the HIP path (``csrc/mcmc.hip``, ``DESIGN.md`` §7.12):
a fixed budget of Gaussians (``cap_max``), dead Gaussians relocated onto live ones with an opacity / scale correction that
keeps the picture, growth by 5 % a round up to the cap, an opacity-gated noise on the positions after every optimizer step
and an L1 prior on opacity and scale.

    loss = loss + mcmc_regularizer(model._opacity, model._scaling, opt.opacity_reg, opt.scale_reg)
    ...
    relocate_gs(model); add_new_gs(model, opt.cap_max)          # on densification iterations
    model.optimizer.step(); inject_noise(model, opt.noise_lr)

``trainer.training_iteration`` does this under ``opt.strategy == "mcmc"``.  Randomness comes in from torch: every function
takes a ``generator`` or the draws themselves.  The model is duck-typed as in ``densify.py``; a model with any fork flag
(``densify.is_fork``) is refused.  There is no CPU path.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .densify import GROUP_ATTR, is_fork, mark_filter_stale, swap_rows_

DRAW_HIGH = 2 ** 63 - 1      # torch.randint's largest exclusive bound: draws are uniform in [0, 2^63 - 1)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _check_model(model, what: str):
    if is_fork(model):
        raise ValueError(f"{what}: the MCMC strategy does not support the fork's grow / learned-split models")
    if not model._xyz.is_cuda:
        raise _lib.GsrError(f"{what} needs ROCm GPU tensors (no CPU path)")
    P = int(model._xyz.shape[0])
    for k, a in GROUP_ATTR.items():
        t = getattr(model, a)
        if t.dtype != torch.float32 or t.shape[0] != P or not t.is_contiguous():
            raise TypeError(f"{k}: expected a contiguous float32 tensor with {P} rows")
    return P


def _need(name: str, t: torch.Tensor) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.GsrError(f"{name} needs a ROCm GPU tensor (no CPU path)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} expects a float32 tensor, got {t.dtype}")


class _McmcReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacity_raw, scaling_raw, opacity_reg: float, scale_reg: float):
        lib = _lib.load()
        oc, sc = opacity_raw.contiguous(), scaling_raw.contiguous()
        P = oc.numel()
        dev = oc.device
        record = torch.zeros(4, dtype=torch.float32, device=dev)      # value, opacity_reg / P, scale_reg / 3P, 0
        ws = torch.empty(lib.gsr_mcmc_reg_workspace_bytes(), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.gsr_mcmc_reg_fwd(oc.data_ptr(), sc.data_ptr(), P, opacity_reg, scale_reg, record.data_ptr(),
                                            ws.data_ptr(), ws.numel(), _stream(dev)), "gsr_mcmc_reg_fwd")
        ctx.save_for_backward(oc, sc, record)
        ctx.shapes = (opacity_raw.shape, scaling_raw.shape)
        return record[0]

    @staticmethod
    def backward(ctx, g):
        oc, sc, record = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()                            # a 0-dim device tensor: never .item()
        go, gs = torch.empty_like(oc), torch.empty_like(sc)
        with torch.cuda.device(oc.device):
            _lib.check(_lib.load().gsr_mcmc_reg_bwd(oc.data_ptr(), sc.data_ptr(), oc.numel(), record.data_ptr(),
                                                    g.data_ptr(), go.data_ptr(), gs.data_ptr(), _stream(oc.device)),
                       "gsr_mcmc_reg_bwd")
        return go.view(ctx.shapes[0]), gs.view(ctx.shapes[1]), None, None


def mcmc_regularizer(opacity_raw: torch.Tensor, scaling_raw: torch.Tensor, opacity_reg: float,
                     scale_reg: float) -> torch.Tensor:
    """``opacity_reg * sigmoid(opacity_raw).mean() + scale_reg * exp(scaling_raw).mean()`` as a 0-dim device tensor with
    dense gradients for both RAW tensors (``[P,1]``, ``[P,3]``): two launches forward, one backward, no read-back, the
    same bits from run to run.  An empty model gives a constant zero."""
    _need("mcmc_regularizer (opacity)", opacity_raw)
    _need("mcmc_regularizer (scaling)", scaling_raw)
    P = opacity_raw.numel()
    if scaling_raw.numel() != 3 * P:
        raise ValueError(f"scaling must hold 3 values per opacity, got {tuple(scaling_raw.shape)} for {P} rows")
    if P == 0:
        return torch.zeros((), dtype=torch.float32, device=opacity_raw.device)
    return _McmcReg.apply(opacity_raw, scaling_raw, float(opacity_reg), float(scale_reg))


def xyz_lr(model) -> float:
    """The current learning rate of the optimizer's ``xyz`` group."""
    for group in model.optimizer.param_groups:
        if group.get("name") == "xyz":
            lr = group["lr"]
            return float(lr.item() if isinstance(lr, torch.Tensor) else lr)
    raise ValueError("the model's optimizer has no 'xyz' group")


def _normal(shape, dev, generator):
    gdev = generator.device if generator is not None else dev
    return torch.randn(shape, dtype=torch.float32, device=gdev, generator=generator).to(dev)


def _uniform_draws(n, dev, generator):
    gdev = generator.device if generator is not None else dev
    return torch.randint(0, DRAW_HIGH, (n,), dtype=torch.int64, device=gdev, generator=generator).to(dev)


@torch.no_grad()
def inject_noise(model, noise_lr: float, generator: Optional[torch.Generator] = None,
                 noise: Optional[torch.Tensor] = None) -> None:
    """``xyz += Sigma (noise * gate(opacity) * noise_lr * lr_xyz)`` in place, one launch (``gsr_mcmc_noise``): ``Sigma``
    the Gaussian's covariance, ``gate = sigmoid(100 ((1 - o) - 0.995))`` -- only nearly transparent Gaussians move.
    The kernel's ``step_scale`` is ``noise_lr * (current lr of the optimizer's "xyz" group)``.
    noise: standard-normal ``[>= P, 3]`` (its first P rows are used); default ``torch.randn`` from ``generator``."""
    P = _check_model(model, "inject_noise")
    if P == 0:
        return
    dev = model._xyz.device
    step_scale = float(noise_lr) * xyz_lr(model)
    if noise is None:
        noise = _normal((P, 3), dev, generator)
    if noise.dim() != 2 or noise.shape[1] != 3 or noise.shape[0] < P:
        raise ValueError(f"noise must be [>= {P}, 3], got {tuple(noise.shape)}")
    noise = noise[:P].to(dev, torch.float32).contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gsr_mcmc_noise(P, model._xyz.data_ptr(), model._scaling.data_ptr(),
                                              model._rotation.data_ptr(), model._opacity.data_ptr(), noise.data_ptr(),
                                              float(step_scale), _stream(dev)), "gsr_mcmc_noise")


def sample_alive(opacity_raw: torch.Tensor, n: int, alive_threshold: float, draws: torch.Tensor):
    """``gsr_mcmc_sample``: ``n`` rows drawn with replacement with probability proportional to ``sigmoid(opacity_raw)``
    among the rows above ``alive_threshold`` (< 0: all rows).  draws: int64 ``[>= n]`` uniform in ``[0, 2^63)``.
    -> ``(idx int32 [n], count int32 [P])``; every ``idx`` is -1 when no row has weight."""
    _need("sample_alive", opacity_raw)
    lib = _lib.load()
    dev = opacity_raw.device
    oc = opacity_raw.detach().contiguous()
    P = oc.numel()
    if draws.dtype != torch.int64 or draws.dim() != 1 or draws.shape[0] < n:
        raise ValueError(f"draws must be int64 [>= {n}], got {draws.dtype} {tuple(draws.shape)}")
    draws = draws[:n].to(dev).contiguous()
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(P, dtype=torch.int32, device=dev)
    ws = torch.empty(max(lib.gsr_mcmc_sample_workspace_bytes(P), 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.gsr_mcmc_sample(P, oc.data_ptr(), float(alive_threshold), draws.data_ptr(), n, idx.data_ptr(),
                                       count.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "gsr_mcmc_sample")
    return idx, count


def relocation(idx: torch.Tensor, count: torch.Tensor, opacity_raw: torch.Tensor, scaling_raw: torch.Tensor):
    """``gsr_mcmc_relocation``: the corrected RAW opacity ``[n,1]`` and scaling ``[n,3]`` of every sample."""
    dev = opacity_raw.device
    n = idx.numel()
    oc, sc = opacity_raw.detach().contiguous(), scaling_raw.detach().contiguous()
    new_o = torch.empty((n, 1), dtype=torch.float32, device=dev)
    new_s = torch.empty((n, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gsr_mcmc_relocation(n, idx.data_ptr(), count.data_ptr(), oc.data_ptr(), sc.data_ptr(),
                                                   new_o.data_ptr(), new_s.data_ptr(), _stream(dev)),
                   "gsr_mcmc_relocation")
    return new_o, new_s


def _zero_moments(model, rows: torch.Tensor, found: Optional[torch.Tensor] = None) -> None:
    """Zeroes exp_avg / exp_avg_sq of ``rows`` in every group (of the rows with ``found`` set, when given)."""
    optimizer = getattr(model, "optimizer", None)
    if optimizer is None:
        return
    for group in optimizer.param_groups:
        if group.get("name") not in GROUP_ATTR:
            continue
        state = optimizer.state.get(group["params"][0], None)
        if state is not None and "exp_avg" in state:
            for key in ("exp_avg", "exp_avg_sq"):
                m = state[key]
                if found is None:
                    m[rows] = 0.0
                else:
                    old = m[rows]
                    m[rows] = torch.where(found.reshape((-1,) + (1,) * (m.dim() - 1)), torch.zeros_like(old), old)


@torch.no_grad()
def relocate_gs(model, dead_threshold: float = 0.005, generator: Optional[torch.Generator] = None,
                draws: Optional[torch.Tensor] = None) -> int:
    """Moves every dead Gaussian (``sigmoid(opacity) <= dead_threshold``) onto a live one sampled by opacity.  With n dead
    rows: sample n sources (``gsr_mcmc_sample``), correct them (``gsr_mcmc_relocation``); every per-Gaussian parameter of
    a dead row becomes its source's, opacity and scaling of the dead row and of the source become the corrected values,
    and the Adam moments of the sources are zeroed (the dead rows keep theirs).  Rows are written in place: P, the
    ``nn.Parameter`` objects and the optimizer's state stay what they are.  Counting the dead rows is the one read-back.
    draws: int64 ``[>= n]`` uniform in ``[0, 2^63)`` (the first n are used); default ``torch.randint`` from ``generator``.
    Returns n (0 also when every row is dead: there is nothing to move onto)."""
    P = _check_model(model, "relocate_gs")
    if P == 0:
        return 0
    dev = model._xyz.device
    # torch's float32 sigmoid is 1 / (1 + exp(-x)), the kernel's expression compiled by the same compiler: the rows
    # found dead here are the rows the sampler gives weight 0 (tests/test_gpu_mcmc.py compares the sampler with a
    # restatement fed by torch.sigmoid, bit for bit).  Should the two ever disagree by an ulp at the threshold, a row
    # is at worst both moved and moved onto; a sample without a source (idx < 0: no row had weight) maps its dead row
    # onto itself with its own values, without a second read-back.
    dead = (torch.sigmoid(model._opacity.detach()).reshape(-1) <= dead_threshold).nonzero(as_tuple=True)[0]
    n = int(dead.numel())                                           # the read-back
    if n == 0 or n == P:
        return 0
    if draws is None:
        draws = _uniform_draws(n, dev, generator)
    idx, count = sample_alive(model._opacity, n, dead_threshold, draws)
    new_o, new_s = relocation(idx, count, model._opacity, model._scaling)
    found = idx >= 0
    mark_filter_stale(model)                                        # dead rows move onto their sources
    src = torch.where(found, idx.long(), dead)
    new_o = torch.where(found[:, None], new_o, model._opacity.detach()[dead])
    new_s = torch.where(found[:, None], new_s, model._scaling.detach()[dead])
    for k, a in GROUP_ATTR.items():
        t = getattr(model, a).detach()
        if k == "opacity":
            t[dead], t[src] = new_o, new_o
        elif k == "scaling":
            t[dead], t[src] = new_s, new_s
        else:
            t[dead] = t[src]
    _zero_moments(model, src, found)
    return n


@torch.no_grad()
def add_new_gs(model, cap_max: int, generator: Optional[torch.Generator] = None,
               draws: Optional[torch.Tensor] = None) -> int:
    """Grows the model by 5 % up to ``cap_max``: ``n = max(0, min(cap_max, int(1.05 P)) - P)`` sources sampled by opacity
    from all rows, corrected as in ``relocate_gs``; the sources take the corrected opacity and scaling and zeroed
    moments, and n copies of them are appended with zero moments and zero densification statistics (the optimizer surgery
    of ``densify.densify_and_prune``).  At the cap it returns 0 and changes nothing.  No read-back.  Returns n."""
    P = _check_model(model, "add_new_gs")
    n = max(0, min(int(cap_max), int(1.05 * P)) - P)
    if n == 0:
        return 0
    dev = model._xyz.device
    if draws is None:
        draws = _uniform_draws(n, dev, generator)
    idx, count = sample_alive(model._opacity, n, -1.0, draws)
    new_o, new_s = relocation(idx, count, model._opacity, model._scaling)
    # idx < 0 (no row has weight: every opacity below 2^-31) has nothing to correct: such a sample copies row 0 as it is,
    # chosen without a read-back
    src = idx.long().clamp_(min=0)
    found = (idx >= 0).reshape(-1, 1)
    new_o = torch.where(found, new_o, model._opacity.detach()[src])
    new_s = torch.where(found, new_s, model._scaling.detach()[src])
    model._opacity.detach()[src] = new_o
    model._scaling.detach()[src] = new_s
    _zero_moments(model, src, found.reshape(-1))
    new = {k: torch.cat([getattr(model, a).detach(), getattr(model, a).detach()[src]], dim=0)
           for k, a in GROUP_ATTR.items()}
    def with_zero_rows(t):
        return torch.cat([t, torch.zeros((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)])
    swap_rows_(model, GROUP_ATTR, new, with_zero_rows)
    for a in ("xyz_gradient_accum", "denom", "max_radii2D", "xyz_gradient_accum_abs"):
        t = getattr(model, a, None)
        if isinstance(t, torch.Tensor) and t.dim() >= 1 and t.shape[0] == P:
            setattr(model, a, with_zero_rows(t))
    return n


__all__ = ["mcmc_regularizer", "inject_noise", "relocate_gs", "add_new_gs", "sample_alive", "relocation", "xyz_lr"]
