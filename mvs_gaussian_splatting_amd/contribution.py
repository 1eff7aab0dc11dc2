"""Which Gaussians the pictures are made of: per-Gaussian blending-weight statistics over a set of views, and pruning
by them -- the measure the compaction recipes since 3DGS rank by (LightGaussian, Mini-Splatting,
RadSplat, Taming-3DGS).

For one rendered frame and Gaussian ``g`` let ``p`` run over the pixels where the colour pass composited ``g`` and
``w = alpha T`` be its blending weight there (the ``w`` the depth / alpha maps sum).  ``ContributionStats.raw`` holds three
int64 per Gaussian: ``sum_p round(w 2^30)``, the number of such pixels, and the float32 bit pattern of ``max_p w``.  The
kernel (``csrc/contribution.hip``) accumulates them with integer adds and an integer max only, so the statistics are the
same bits from run to run, additive over views, and many views accumulate on the device with nothing going to the host:

    stats = measure(model, cameras, pipe, background)            # or render(..., contribution=stats) frame by frame
    prune_by_contribution(model, stats, kind="sum", keep_ratio=0.5)

``2^63 / 2^30`` weight units per Gaussian are about 4000 fully covered 1920x1080 frames.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from .layout import prune_points_
from .renderer import render

FX_ONE = 1 << 30      # the fixed-point unit of raw[:, 0]
KINDS = ("sum", "max", "count", "mean")


class ContributionStats:
    """The accumulator of ``render(..., contribution=stats)`` / ``GaussianRasterizer(settings, contribution=stats)``:
    ``raw`` int64 ``[P,3]`` (fixed-point weight sum, pixel count, bits of the largest weight) and ``views``, the number
    of frames added so far."""

    def __init__(self, P: int, device=None):
        self.raw = torch.zeros((int(P), 3), dtype=torch.int64, device=device)
        self.views = 0

    def weight_sum(self) -> torch.Tensor:
        """float64 ``[P]``: the sum of the blending weights (each rounded to ``2^-30``)."""
        return self.raw[:, 0].to(torch.float64) / FX_ONE

    def pixel_count(self) -> torch.Tensor:
        """int64 ``[P]``: the number of (view, pixel) pairs the Gaussian was composited at."""
        return self.raw[:, 1].clone()

    def max_weight(self) -> torch.Tensor:
        """float32 ``[P]``: the largest blending weight (0 for a Gaussian never composited)."""
        return self.raw[:, 2].to(torch.int32).view(torch.float32)

    def score(self, kind: str = "sum") -> torch.Tensor:
        """``"sum"`` (float64), ``"max"`` (float32), ``"count"`` (int64) or ``"mean"`` = sum / max(count, 1) (float64)."""
        if kind == "sum":
            return self.weight_sum()
        if kind == "max":
            return self.max_weight()
        if kind == "count":
            return self.pixel_count()
        if kind == "mean":
            return self.weight_sum() / self.raw[:, 1].clamp(min=1).to(torch.float64)
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")

    def reset(self) -> None:
        self.raw.zero_()
        self.views = 0

    def merge(self, other: "ContributionStats") -> "ContributionStats":
        """Add another accumulator of the same model into this one: add, add, max; the views add up."""
        if tuple(other.raw.shape) != tuple(self.raw.shape):
            raise ValueError(f"cannot merge statistics of {int(other.raw.shape[0])} Gaussians into {int(self.raw.shape[0])}")
        o = other.raw.to(self.raw.device)
        self.raw[:, :2] += o[:, :2]
        self.raw[:, 2] = torch.maximum(self.raw[:, 2], o[:, 2])
        self.views += other.views
        return self


def measure(model, cameras: Sequence, pipe, background: torch.Tensor, *, masks: Optional[Sequence] = None
            ) -> ContributionStats:
    """Render every camera under ``no_grad`` and accumulate the statistics of the frames.  ``masks``: None, or one
    entry per camera, each None or a uint8 ``[H,W]`` device tensor whose zero pixels are left out.  The loop adds no
    host synchronisation to the frames' own."""
    if masks is not None and len(masks) != len(cameras):
        raise ValueError(f"masks has {len(masks)} entries for {len(cameras)} cameras")
    stats = ContributionStats(int(model._xyz.shape[0]), model._xyz.device)
    with torch.no_grad():
        for i, camera in enumerate(cameras):
            render(camera, model, pipe, background, contribution=stats,
                   contribution_mask=None if masks is None else masks[i])
    return stats


def prune_by_contribution(model, stats: ContributionStats, *, kind: str = "sum", keep_ratio: Optional[float] = None,
                          min_score: Optional[float] = None) -> dict:
    """Drop the Gaussians that contribute least (``layout.prune_points_``).  Exactly one of:
    ``keep_ratio``: the ``ceil(keep_ratio * P)`` highest ``stats.score(kind)`` stay, ties broken by the lower index;
    ``min_score``: the rows with ``score >= min_score`` stay.
    Returns ``{"points": rows left, "pruned": rows removed}``."""
    if (keep_ratio is None) == (min_score is None):
        raise ValueError("give exactly one of keep_ratio and min_score")
    P = int(model._xyz.shape[0])
    if int(stats.raw.shape[0]) != P:
        raise ValueError(f"the statistics have {int(stats.raw.shape[0])} rows, the model has P={P} Gaussians")
    score = stats.score(kind)
    if keep_ratio is not None:
        if not 0.0 <= keep_ratio <= 1.0:
            raise ValueError(f"keep_ratio must be in [0, 1], got {keep_ratio}")
        n_keep = min(P, math.ceil(keep_ratio * P - 1e-9))      # 0.1 * 30 is 3.0000000000000004 in binary: still 3 rows
        order = torch.sort(score, descending=True, stable=True).indices      # stable: equal scores stay in index order
        keep = torch.zeros(P, dtype=torch.bool, device=score.device)
        keep[order[:n_keep]] = True
    else:
        keep = score >= min_score
    left = prune_points_(model, keep)
    return {"points": left, "pruned": P - left}


__all__ = ["ContributionStats", "measure", "prune_points_", "prune_by_contribution", "KINDS"]
