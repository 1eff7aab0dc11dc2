"""Per-Gaussian feature vectors for the rasterizer's ``features=`` input (``rasterizer.py``), in plain
torch.  ``gaussian_normals`` is the one consumer shipped: the normal of a Gaussian taken as a flat disc."""
from __future__ import annotations

import torch


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
