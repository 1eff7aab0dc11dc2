"""Per-Gaussian feature vectors for the rasterizer's ``features=`` input (``rasterizer.py``).
``gaussian_normals``, in plain torch: the normal of a Gaussian taken as a flat disc.  ``gaussian_planes``, one HIP launch
each way (``csrc/planes.hip``): that normal and the distance of the camera centre from the disc's plane,
the rows PGSR's unbiased depth is rendered from."""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib


def _rotation_matrices(rotations: torch.Tensor) -> torch.Tensor:
    """[P,3,3] rotation matrices of quaternions (r, x, y, z) -- the rasterizer's convention -- normalised first."""
    q = torch.nn.functional.normalize(rotations, dim=1)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = (1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y),
            2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x),
            2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y))
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def gaussian_normals(scales: torch.Tensor, rotations: torch.Tensor, means3D: torch.Tensor, viewmatrix: torch.Tensor,
                     campos: torch.Tensor) -> torch.Tensor:
    """View-space unit normals ``[P,3]`` of the Gaussians: the column of the rotation matrix that belongs to the smallest
    scale (the axis the Gaussian is flattest along), its sign flipped so that it faces the camera
    (``n . (campos - mean) >= 0``), rotated into view space with the row-vector convention of
    ``GaussianRasterizationSettings`` (``n_view = n_world @ viewmatrix[:3,:3]``).  Differentiable in ``rotations``; which
    axis is the smallest and the sign are decisions and carry no gradient."""
    R = _rotation_matrices(rotations)
    axis = torch.argmin(scales.detach(), dim=1)
    n = torch.gather(R, 2, axis.view(-1, 1, 1).expand(-1, 3, 1)).squeeze(2)
    facing = (n.detach() * (campos.detach().view(1, 3) - means3D.detach())).sum(dim=1)
    n = n * torch.where(facing < 0, -1.0, 1.0).to(n.dtype).unsqueeze(1)
    return n @ viewmatrix[:3, :3].to(n.dtype)


def _check_planes(scales, rotations, means3D, viewmatrix, campos):
    """Every refusal of ``gaussian_planes``, before anything is enqueued and before a GPU is asked for.  Returns P."""
    what = "gaussian_planes"
    named = (("scales", scales, 3), ("rotations", rotations, 4), ("means3D", means3D, 3))
    for name, t, _ in named + (("viewmatrix", viewmatrix, 0), ("campos", campos, 0)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32, got {t.dtype}")
    P = int(rotations.shape[0]) if rotations.dim() == 2 else -1
    for name, t, width in named:
        if t.dim() != 2 or tuple(t.shape) != (P, width):
            raise ValueError(f"{what}: {name} must be [P,{width}] with the P of rotations, got {tuple(t.shape)}")
        if t.device != rotations.device:
            raise ValueError(f"{what}: rotations is on {rotations.device}, {name} on {t.device}")
    if P > 2 ** 31 - 1:
        raise ValueError(f"{what}: at most 2^31 - 1 rows, got {P}")
    if tuple(viewmatrix.shape) != (4, 4):
        raise ValueError(f"{what}: viewmatrix must be [4,4], got {tuple(viewmatrix.shape)}")
    if campos.numel() != 3:
        raise ValueError(f"{what}: campos must hold 3 numbers, got {tuple(campos.shape)}")
    if viewmatrix.requires_grad or campos.requires_grad:
        raise ValueError(f"{what}: viewmatrix and campos must not require a gradient (camera gradients are not "
                         "computed here; the trainer refuses geometry terms together with pose_optimizer)")
    if not rotations.is_cuda:
        raise _lib.GsrError(f"{what} needs ROCm GPU tensors (no CPU path)")
    return P


def _host_floats(t: torch.Tensor, n: int):
    """``t`` as ``n`` host floats.  The copy is kept on the tensor object with the version it was taken at, so a camera
    whose matrices are the same tensors from frame to frame is read back once, not once per call (a device-to-host
    copy drains the stream); an in-place write bumps the version and the next call copies again."""
    cached = getattr(t, "_gsr_host_floats", None)
    if cached is not None and cached[0] == t._version:
        return cached[1]
    host = (ctypes.c_float * n)(*t.detach().to("cpu").reshape(n).tolist())
    try:
        t._gsr_host_floats = (t._version, host)
    except (AttributeError, RuntimeError):      # a tensor that takes no attributes is copied every time
        pass
    return host


def _host_camera(viewmatrix: torch.Tensor, campos: torch.Tensor):
    """(viewmatrix as 16 host floats, campos as 3): the kernels take the camera as launch arguments."""
    return _host_floats(viewmatrix, 16), _host_floats(campos, 3)


def planes_forward_raw(scales, rotations, means3D, vm, cp, out=None) -> torch.Tensor:
    """``gsr_gaussian_planes_fwd`` on contiguous device tensors and a host camera (``_host_camera``) -> ``[P,4]``."""
    lib = _lib.load()
    P = int(rotations.shape[0])
    planes = torch.empty((P, 4), dtype=torch.float32, device=rotations.device) if out is None else out
    with torch.cuda.device(rotations.device):
        stream = torch.cuda.current_stream(rotations.device).cuda_stream
        _lib.check(lib.gsr_gaussian_planes_fwd(scales.data_ptr(), rotations.data_ptr(), means3D.data_ptr(), P,
                                               ctypes.addressof(vm), ctypes.addressof(cp), planes.data_ptr(), stream),
                   "gsr_gaussian_planes_fwd")
    return planes


def planes_backward_raw(scales, rotations, means3D, vm, cp, grad, out=None):
    """``gsr_gaussian_planes_bwd`` -> ``(dL/drotations [P,4], dL/dmeans3D [P,3])``."""
    lib = _lib.load()
    P = int(rotations.shape[0])
    d_rot, d_mean = (torch.empty_like(rotations), torch.empty_like(means3D)) if out is None else out
    with torch.cuda.device(rotations.device):
        stream = torch.cuda.current_stream(rotations.device).cuda_stream
        _lib.check(lib.gsr_gaussian_planes_bwd(scales.data_ptr(), rotations.data_ptr(), means3D.data_ptr(), P,
                                               ctypes.addressof(vm), ctypes.addressof(cp), grad.data_ptr(),
                                               d_rot.data_ptr(), d_mean.data_ptr(), stream), "gsr_gaussian_planes_bwd")
    return d_rot, d_mean


class _GaussianPlanes(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scales, rotations, means3D, vm, cp):
        sc, rc, mc = scales.detach().contiguous(), rotations.detach().contiguous(), means3D.detach().contiguous()
        if rc.data_ptr() % 16:                   # a view into a larger block: the kernel loads the row as 16 bytes
            rc = rc.clone()
        ctx.save_for_backward(sc, rc, mc)
        ctx.camera = (vm, cp)
        return planes_forward_raw(sc, rc, mc, vm, cp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        sc, rc, mc = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        if g.data_ptr() % 16:
            g = g.clone()
        d_rot, d_mean = planes_backward_raw(sc, rc, mc, *ctx.camera, g)
        return None, d_rot if ctx.needs_input_grad[1] else None, d_mean if ctx.needs_input_grad[2] else None, None, None


def gaussian_planes(scales: torch.Tensor, rotations: torch.Tensor, means3D: torch.Tensor, viewmatrix: torch.Tensor,
                    campos: torch.Tensor) -> torch.Tensor:
    """Per-Gaussian planes ``[P,4]`` = ``(n_view, d)``: ``n_view`` the view-space unit normal of ``gaussian_normals``
    (the rotation-matrix column of the smallest scale, the smallest index among equal scales, facing the camera, a
    facing dot product of exactly 0 keeping ``+1``) and ``d = n_world . (campos - mean) >= 0``, the distance of the
    camera centre from the Gaussian's plane.  Composited as four feature channels they give ``N = sum w n`` and ``D =
    sum w d``, from which ``surface.plane_depth`` takes PGSR's unbiased depth.  One HIP launch forward and one backward
    (float32 ``[P,3]``, ``[P,4]``, ``[P,3]`` on one GPU; ``GsrError`` on CPU tensors); differentiable in ``rotations`` and
    ``means3D`` (once: there is no double backward), the axis and the sign being decisions without gradient; the same
    bits from run to run.  ``viewmatrix`` and ``campos`` are copied to the host (the kernels take them as launch
    arguments) the first time each tensor is seen and again after an in-place write to it -- one synchronisation per
    camera, not per call -- and must not require a gradient: ``ValueError``.  ``[:, :3]`` may differ from ``gaussian_normals`` in the last bits (the kernel rounds once)."""
    _check_planes(scales, rotations, means3D, viewmatrix, campos)
    return _GaussianPlanes.apply(scales, rotations, means3D, *_host_camera(viewmatrix, campos))
