"""Spatial ordering of the Gaussians in memory (an optional layout step; not part of the reference's path).

The kernels stream the per-Gaussian tensors by index: lane i of a wave handles Gaussian i.  Whether a Gaussian is inside
the frustum, and which tiles it reaches, depends on where it IS -- so when neighbours in memory are neighbours in space,
whole waves are culled together (their 192-byte SH rows are skipped as whole lines instead of leaving half-used lines
behind), the instance lists of a tile point at adjacent 64-byte records and the gradient rows of a wave's Gaussians are
adjacent too.  The reference appends clones and split children at the end of its tensors
(``scene/gaussian_model.py:466-504``), so a model under training is in no spatial order.  ``reorder_gaussians_`` stores
it along a 30-bit Morton curve of the positions, with the Adam-moment surgery of the reference's ``_prune_optimizer``
(``:401-417``: same groups, same state keys); a trainer calls it after ``densify_and_prune`` (every 100 iterations,
``train.py:130-134``).

Results are the unpermuted model's up to the permutation: every per-Gaussian quantity is computed from that Gaussian's
row alone, and a tile's list is ordered by depth.  Only equal-depth ties inside a tile (broken by index, as in the
reference's stable sort) can blend in another order; a frame without such ties is bit-identical, gradients included
(``tests/test_gpu_layout.py``; at 6 M Gaussians the sorted keys are the same array, 882 of 8.2 M list entries swap places
inside equal-key runs and 279 of 2 M pixels differ, by at most 1.2e-3).  Measured on the 6 M-Gaussian bench cloud, whose index order is uniformly random:
forward 0.912 -> 0.846 ms, train step 2.252 -> 2.056 ms (``profiles/r04/layout_morton.txt``).
"""
from __future__ import annotations

from typing import Optional

import torch

from .densify import FORK_ATTR, GROUP_ATTR, swap_rows_

STATS_ATTR = ("xyz_gradient_accum", "denom", "max_radii2D", "xyz_gradient_accum_abs")


def _spread3(v: torch.Tensor) -> torch.Tensor:
    """10-bit integers -> their bits spread to every third position (int64)."""
    v = v & 0x3ff
    v = (v | (v << 16)) & 0x030000ff
    v = (v | (v << 8)) & 0x0300f00f
    v = (v | (v << 4)) & 0x030c30c3
    v = (v | (v << 2)) & 0x09249249
    return v


@torch.no_grad()
def morton_permutation(xyz: torch.Tensor) -> torch.Tensor:
    """Indices that sort the points along a 30-bit Morton (Z-order) curve over their bounding box; points of one cell keep
    their order (stable).  ``xyz``: ``[P, 3]`` on any device."""
    p = xyz.detach().float()
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError(f"xyz must be [P, 3], got {tuple(p.shape)}")
    if p.shape[0] == 0:
        return torch.empty(0, dtype=torch.int64, device=p.device)
    lo, hi = p.min(dim=0).values, p.max(dim=0).values
    q = ((p - lo) / (hi - lo).clamp(min=1e-12) * 1023.0).clamp(0.0, 1023.0).to(torch.int64)
    code = _spread3(q[:, 0]) | (_spread3(q[:, 1]) << 1) | (_spread3(q[:, 2]) << 2)
    return torch.sort(code, stable=True).indices


def _take_rows_(model, index: torch.Tensor, P: int) -> None:
    """Row ``index`` (an int64 index or a bool mask over the P rows) of every per-Gaussian tensor of the model, in place:
    the parameter tensors, the fork's learned tensors with one row per Gaussian, the Adam moments of ``model.optimizer``
    (the surgery of the reference's ``_prune_optimizer``: same groups, same state keys) and the densification
    statistics."""
    attrs = dict(GROUP_ATTR)
    for k, a in FORK_ATTR.items():
        t = getattr(model, a, None)
        if isinstance(t, torch.Tensor) and t.dim() >= 1 and t.shape[0] == P and P > 0:
            attrs[k] = a
    def take(t):
        return t.detach()[index].contiguous()
    swap_rows_(model, attrs, {k: take(getattr(model, a)) for k, a in attrs.items()}, take)
    for a in STATS_ATTR:
        t = getattr(model, a, None)
        if isinstance(t, torch.Tensor) and t.dim() >= 1 and t.shape[0] == P:
            setattr(model, a, t[index].contiguous())


@torch.no_grad()
def reorder_gaussians_(model, perm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Permute every per-Gaussian tensor of a model in place: row i of the result is row ``perm[i]`` of the input
    (default: ``morton_permutation(model._xyz)``).  The model is duck-typed as in ``densify.py``: the six parameter
    tensors, the fork's learned tensors (``FORK_ATTR``) that have one row per Gaussian, the densification statistics if
    present, and ``model.optimizer`` (one parameter per named group) if present,
    whose ``exp_avg`` / ``exp_avg_sq`` rows move with their Gaussians.  Returns the permutation."""
    xyz = model._xyz
    P = int(xyz.shape[0])
    if perm is None:
        perm = morton_permutation(xyz)
    perm = perm.to(device=xyz.device, dtype=torch.int64)
    if perm.shape != (P,) or (P and not torch.equal(torch.sort(perm).values, torch.arange(P, device=perm.device))):
        raise ValueError(f"perm must be a permutation of range({P})")
    _take_rows_(model, perm, P)
    return perm


@torch.no_grad()
def prune_points_(model, keep: torch.Tensor) -> int:
    """Keep the Gaussians a bool ``[P]`` mask marks and drop the rest, in place and in order: the rows of everything
    ``reorder_gaussians_`` moves (parameters, the fork's learned tensors, the Adam moments, the densification
    statistics); the kept rows keep their bits.  Per-image exposures have no row per Gaussian and are untouched.  Plain
    torch indexing -- a cold path -- so it also serves a model on the CPU.  Returns the number of points left."""
    xyz = model._xyz
    P = int(xyz.shape[0])
    if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or tuple(keep.shape) != (P,):
        raise ValueError(f"keep must be a bool [P={P}] mask, got "
                         f"{getattr(keep, 'dtype', type(keep).__name__)} {list(getattr(keep, 'shape', ()))}")
    _take_rows_(model, keep.to(xyz.device), P)
    return int(model._xyz.shape[0])
