"""Per-image bilateral grids: the appearance correction of "Bilateral Guided Radiance Field Processing" (gsplat's
``--use_bilateral_grid``) on the HIP path (``csrc/bilagrid.hip`` behind ``gsr_bilagrid_*``).

    grids = BilateralGrids([cam.image_name for cam in train_cameras])
    grids.training_setup(opt)
    loss = training_iteration(gaussians, camera, opt, pipe, background, iteration, cameras_extent=extent,
                              bilateral_grids=grids)

Each training image owns a grid ``[12,L,Hg,Wg]`` of 3x4 colour affines (channel ``4 c + k`` is ``A[c,k]``, ``c`` the
output colour, ``k`` the input colour, ``k = 3`` the offset), indexed by the pixel's position and by the rendered pixel's
own luminance, sliced trilinearly and applied to the render before the colour loss: local tone mapping, white balance
and vignetting are explained there, where a global exposure cannot follow them and the Gaussians would answer with
floaters.  The identity grid returns the image and passes the gradient through bit for bit, so a run that starts there
begins exactly as a run without grids.  ``dL/dgrid`` and the total-variation term are summed in double in a fixed order:
the same bits from run to run.
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch

from . import _lib
from .optim import Adam, expon_lr_func

DEFAULT_SHAPE = (16, 16, 8)                  # (Wg, Hg, L)
_MAX_XY, _MAX_L = 64, 16


def _check_grid_sizes(what: str, Wg: int, Hg: int, L: int) -> None:
    if not (2 <= Wg <= _MAX_XY and 2 <= Hg <= _MAX_XY and 2 <= L <= _MAX_L):
        raise ValueError(f"{what}: the grid must hold 2..{_MAX_XY} x 2..{_MAX_XY} x 2..{_MAX_L} vertices (Wg, Hg, L), got "
                         f"{Wg} x {Hg} x {L}")


def _check_slice(image, grid):
    """Every refusal, before anything is enqueued and before a GPU is asked for.  Returns (H, W, Wg, Hg, L)."""
    what = "slice_bilateral_grid"
    for name, t in (("image", image), ("grid", grid)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32, got {t.dtype}")
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"{what}: image must be [3,H,W], got {tuple(image.shape)}")
    if grid.dim() != 4 or grid.shape[0] != 12:
        raise ValueError(f"{what}: grid must be [12,L,Hg,Wg], got {tuple(grid.shape)}")
    H, W = int(image.shape[1]), int(image.shape[2])
    if H < 1 or W < 1 or H * W > 1 << 28:
        raise ValueError(f"{what}: the image must hold between 1 and 2^28 pixels, got {H} x {W}")
    L, Hg, Wg = (int(v) for v in grid.shape[1:])
    _check_grid_sizes(what, Wg, Hg, L)
    if image.device != grid.device:
        raise ValueError(f"{what}: the image is on {image.device}, the grid on {grid.device}")
    if not image.is_cuda:
        raise _lib.GsrError(f"{what} needs ROCm GPU tensors (no CPU path)")
    return H, W, Wg, Hg, L


class _SliceBilateralGrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, grid, sizes):
        lib = _lib.load()
        H, W, Wg, Hg, L = sizes
        xc, gc = image.contiguous(), grid.contiguous()
        y = torch.empty_like(xc)
        with torch.cuda.device(xc.device):
            stream = torch.cuda.current_stream(xc.device).cuda_stream
            _lib.check(lib.gsr_bilagrid_slice_fwd(xc.data_ptr(), gc.data_ptr(), H, W, Wg, Hg, L, _lib.BILAGRID_STAGE_AUTO,
                                                  y.data_ptr(), stream), "gsr_bilagrid_slice_fwd")
        ctx.save_for_backward(xc, gc)
        ctx.sizes = sizes
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        xc, gc = ctx.saved_tensors
        need_dx, need_dg = ctx.needs_input_grad[:2]
        if not (need_dx or need_dg):
            return None, None, None
        H, W, Wg, Hg, L = ctx.sizes
        g = g.to(torch.float32).contiguous()
        dx = torch.empty_like(xc) if need_dx else None
        dg = ws = None
        if need_dg:
            dg = torch.empty_like(gc)
            ws = torch.empty(lib.gsr_bilagrid_workspace_bytes(H, W, Wg, Hg, L), dtype=torch.uint8, device=xc.device)
        ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
        with torch.cuda.device(xc.device):
            stream = torch.cuda.current_stream(xc.device).cuda_stream
            _lib.check(lib.gsr_bilagrid_slice_bwd(xc.data_ptr(), gc.data_ptr(), g.data_ptr(), H, W, Wg, Hg, L,
                                                  _lib.BILAGRID_STAGE_AUTO, ptr(dx), ptr(dg), ptr(ws), stream),
                       "gsr_bilagrid_slice_bwd")
        return dx, dg, None


def slice_bilateral_grid(image: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
    """``image`` float32 ``[3,H,W]`` and ``grid`` float32 ``[12,L,Hg,Wg]`` (``2 <= Wg, Hg <= 64``, ``2 <= L <= 16``) on
    one GPU, made contiguous if they are not; returns the ``[3,H,W]`` image after the affine the grid holds at each
    pixel's position and luminance (module docstring), without a clamp.  Differentiable in both, the image also through
    its luminance; a gradient is computed only for the input that requires one.  Nothing is read back."""
    sizes = _check_slice(image, grid)
    return _SliceBilateralGrid.apply(image, grid, sizes)


class _TvLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        lib = _lib.load()
        gc = grids.contiguous()
        N, _, L, Hg, Wg = (int(v) for v in gc.shape)
        need = ctx.needs_input_grad[0]
        value = torch.empty(1, dtype=torch.float32, device=gc.device)
        unit = torch.empty_like(gc) if need else None
        ws = torch.empty(lib.gsr_bilagrid_workspace_bytes(0, 0, Wg, Hg, L), dtype=torch.uint8, device=gc.device)
        with torch.cuda.device(gc.device):
            stream = torch.cuda.current_stream(gc.device).cuda_stream
            _lib.check(lib.gsr_bilagrid_tv_fwd_bwd(gc.data_ptr(), N, Wg, Hg, L, value.data_ptr(),
                                                   None if unit is None else unit.data_ptr(), ws.data_ptr(), stream),
                       "gsr_bilagrid_tv_fwd_bwd")
        if need:
            ctx.save_for_backward(unit)
        return value[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (unit,) = ctx.saved_tensors
        return unit * g.to(torch.float32)                            # a 0-dim device tensor: never .item()


def bilateral_grid_tv_loss(grids: torch.Tensor) -> torch.Tensor:
    """gsplat's ``total_variation_loss`` of ``grids`` float32 ``[N,12,L,Hg,Wg]`` on a GPU: ``(1/N) sum_n sum_axis
    mean((grids[n] shifted by one along the axis - grids[n])^2)`` over the axes z, y and x, as a 0-dim device tensor.
    One launch computes the value and, when ``grids`` requires one, its gradient.  Nothing is read back."""
    what = "bilateral_grid_tv_loss"
    if not isinstance(grids, torch.Tensor):
        raise TypeError(f"{what}: grids must be a torch.Tensor, got {type(grids).__name__}")
    if grids.dtype != torch.float32:
        raise TypeError(f"{what}: grids must be float32, got {grids.dtype}")
    if grids.dim() != 5 or grids.shape[1] != 12:
        raise ValueError(f"{what}: grids must be [N,12,L,Hg,Wg], got {tuple(grids.shape)}")
    N, _, L, Hg, Wg = (int(v) for v in grids.shape)
    if not 1 <= N <= 1 << 16:
        raise ValueError(f"{what}: between 1 and 65536 grids, got {N}")
    _check_grid_sizes(what, Wg, Hg, L)
    if not grids.is_cuda:
        raise _lib.GsrError(f"{what} needs ROCm GPU tensors (no CPU path)")
    return _TvLoss.apply(grids)


class BilateralGrids:
    """One learnable bilateral grid per training image, at the identity: ``grids`` is a parameter ``[N,12,L,Hg,Wg]``
    and ``mapping`` takes an image name to its row.  ``shape`` is ``(Wg, Hg, L)``.  device: default the current ROCm
    device (a CPU device is accepted: the tensor is host data until it is sliced).  It lives beside the model, with an
    optimizer and files of its own: ``GaussianModel.capture()`` does not know it."""

    def __init__(self, image_names: Sequence[str], shape=DEFAULT_SHAPE, device=None):
        names = list(image_names)
        if not names:
            raise ValueError("BilateralGrids needs at least one image name")
        if len(set(names)) != len(names):
            raise ValueError("BilateralGrids needs distinct image names")
        if len(names) > 1 << 16:
            raise ValueError(f"BilateralGrids holds at most 65536 images, got {len(names)}")
        try:
            Wg, Hg, L = (int(v) for v in shape)
        except (TypeError, ValueError):
            raise ValueError(f"BilateralGrids: shape must be (Wg, Hg, L), got {shape!r}") from None
        _check_grid_sizes("BilateralGrids", Wg, Hg, L)
        eye = torch.eye(3, 4, dtype=torch.float32, device="cuda" if device is None else device)
        cell = eye.reshape(12, 1, 1, 1).expand(12, L, Hg, Wg)
        self.shape = (Wg, Hg, L)
        self.grids = torch.nn.Parameter(cell[None].repeat(len(names), 1, 1, 1, 1).contiguous().requires_grad_(True))
        self.mapping: Dict[str, int] = {name: i for i, name in enumerate(names)}
        self.optimizer = None
        self.scheduler_args = None

    def grid_for(self, image_name) -> torch.Tensor:
        """The ``[12,L,Hg,Wg]`` grid of one image: a view of its row of ``grids`` (the gradient lands there).
        ``KeyError`` for a name that has none."""
        if image_name not in self.mapping:
            raise KeyError(f"no bilateral grid for image {image_name!r}")
        return self.grids[self.mapping[image_name]]

    def training_setup(self, opt):
        """``optim.Adam([grids], lr=0.0, eps=1e-15)`` and the exponential schedule from ``opt.bilateral_grid_lr_init`` to
        ``opt.bilateral_grid_lr_final`` over ``opt.iterations`` steps.  Returns the optimizer."""
        self.optimizer = Adam([self.grids], lr=0.0, eps=1e-15)
        self.scheduler_args = expon_lr_func(float(getattr(opt, "bilateral_grid_lr_init", 2e-3)),
                                            float(getattr(opt, "bilateral_grid_lr_final", 2e-5)),
                                            max_steps=int(opt.iterations))
        return self.optimizer

    def update_learning_rate(self, iteration):
        if self.optimizer is None:
            raise ValueError("BilateralGrids.update_learning_rate needs training_setup first")
        lr = self.scheduler_args(iteration)
        for group in self.optimizer.param_groups:
            group["lr"] = lr
        return lr

    def state_dict(self) -> dict:
        return {"grids": self.grids.detach().clone(), "mapping": dict(self.mapping), "shape": tuple(self.shape),
                "optimizer": None if self.optimizer is None else self.optimizer.state_dict()}

    def load_state_dict(self, state) -> None:
        """Takes what ``state_dict`` returned.  ``ValueError`` when the names or the shape differ from this object's, or
        when the state holds an optimizer and ``training_setup`` has not run."""
        for key in ("grids", "mapping", "shape", "optimizer"):
            if key not in state:
                raise ValueError(f"BilateralGrids.load_state_dict: the state has no {key!r}")
        if dict(state["mapping"]) != self.mapping or tuple(state["shape"]) != tuple(self.shape):
            raise ValueError("BilateralGrids.load_state_dict: the state was saved for other images or another grid shape")
        grids = state["grids"]
        if not isinstance(grids, torch.Tensor) or grids.dtype != torch.float32 or grids.shape != self.grids.shape:
            raise ValueError(f"BilateralGrids.load_state_dict: grids must be float32 {tuple(self.grids.shape)}")
        if state["optimizer"] is not None and self.optimizer is None:
            raise ValueError("BilateralGrids.load_state_dict: the state holds an optimizer; call training_setup first")
        with torch.no_grad():
            self.grids.copy_(grids)
        if state["optimizer"] is not None:
            self.optimizer.load_state_dict(state["optimizer"])

    def save(self, path: str) -> None:
        """``torch.save(state_dict(), path)``."""
        torch.save(self.state_dict(), path)

    def load(self, path: str) -> None:
        """``load_state_dict`` of a file ``save`` wrote.  The file is a pickle of tensors, numbers and the optimizer's
        state dict: load only files you wrote."""
        self.load_state_dict(torch.load(path, map_location=self.grids.device, weights_only=False))


__all__ = ["slice_bilateral_grid", "bilateral_grid_tv_loss", "BilateralGrids"]
