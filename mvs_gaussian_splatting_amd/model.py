"""The reference's ``GaussianModel`` (``scene/gaussian_model.py``) for the HIP path: the object that ``render``,
``add_densification_stats``, ``densify.densify_and_prune``, ``optim.training_setup``, ``layout.reorder_gaussians_``,
``ply_io.save_ply`` and ``evaluate_views`` are handed, with the lifecycle around them -- initialisation from a point
cloud (``create_from_pcd`` ``:200-238``), ``oneupSHdegree`` (``:196-198``), ``reset_opacity`` (``:312-315``),
checkpoints (``capture`` / ``restore`` ``:84-149``) and PLY files (``:293-358``).

    gaussians = GaussianModel(sh_degree, grow_dir=..., num_dirs=..., continous_dir=..., grow_distance=..., modelcg=dataset)
    gaussians.create_from_pcd(pcd.points, pcd.colors, cameras_extent)
    gaussians.training_setup(opt)

Same constructor, attribute names and getters as the reference, so code written against its class runs unchanged;
densification stays the function ``densify.densify_and_prune(gaussians, ...)`` and the statistics
``add_densification_stats(gaussians, ...)`` (``trainer.training_iteration`` calls both in the reference's order).
There is no CPU path: the methods that compute raise ``GsrError`` on CPU tensors; constructing a model, ``capture`` and
``oneupSHdegree`` are host code and run anywhere.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from . import _lib, filter3d, knn, optim, ply_io
from .densify import FORK_ATTR, FORK_FLAG, GROUP_ATTR
from .sh import RGB2SH

RESET_OPACITY_CAP = 0.01            # scene/gaussian_model.py:313
INITIAL_OPACITY = 0.1               # :215
MIN_DIST2 = 0.0000001               # :210


def sphere_points(n: int = 128) -> np.ndarray:
    """``utils/general_utils.py:135-148``: ``n`` directions on a golden-angle spiral over the unit sphere, float64
    ``[n, 3]``, from ``z = 1 - 1/n`` down to ``1/n - 1``."""
    golden_angle = np.pi * (3.0 - np.sqrt(5.0))
    theta = golden_angle * np.arange(n)
    z = np.linspace(1 - 1.0 / n, 1.0 / n - 1, n)
    radius = np.sqrt(1 - z * z)
    return np.stack((radius * np.cos(theta), radius * np.sin(theta), z), axis=1)


def inverse_sigmoid(x: torch.Tensor) -> torch.Tensor:
    """``utils/general_utils.py:18-19``."""
    return torch.log(x / (1 - x))


def covariance_from_scaling_rotation(scaling, scaling_modifier, rotation):
    """``scene/gaussian_model.py:28-32``: the six unique entries of ``(R S)(R S)^T``, ``[P, 6]``, from activated scales
    and raw quaternions."""
    s = scaling_modifier * scaling
    q = torch.nn.functional.normalize(rotation)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    L = R * s[:, None, :]
    cov = L @ L.transpose(1, 2)
    return torch.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], dim=1)


checked_filter_3D = filter3d.checked_filter_3D


def _required_filter(pc, what: str):
    f = checked_filter_3D(pc, what)
    if f is None:
        raise ValueError(f"{what}: the model has no 3D filter; call compute_3D_filter(cameras) first")
    return f


class _Fused:
    """What ``ply_io.save_ply`` reads of a model, with the effective raw scales and opacities in place of its own."""

    def __init__(self, model, scaling, opacity):
        self._xyz, self._features_dc, self._features_rest = model._xyz, model._features_dc, model._features_rest
        self._rotation, self._scaling, self._opacity = model._rotation, scaling, opacity


def _need_gpu(name: str, t: torch.Tensor) -> None:
    if not t.is_cuda:
        raise _lib.GsrError(f"{name} needs ROCm GPU tensors (no CPU path)")


class GaussianModel:
    """See the module docstring.  ``modelcg`` is the reference's dataset namespace (``learn_split_distance``,
    ``learn_split_scale``, ``symmetric_split``, ``split_notreinit``, ``prob_notreinit``); None means no learned split."""

    def __init__(self, sh_degree: int, grow_dir=False, num_dirs=128, continous_dir=False, grow_distance=False,
                 modelcg=None):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        self._xyz = torch.empty(0)
        self._features_dc = torch.empty(0)
        self._features_rest = torch.empty(0)
        self._scaling = torch.empty(0)
        self._rotation = torch.empty(0)
        self._opacity = torch.empty(0)
        self.max_radii2D = torch.empty(0)
        self.xyz_gradient_accum = torch.empty(0)
        self.denom = torch.empty(0)
        self.xyz_gradient_accum_abs = None      # AbsGS / PGSR's accumulator [P,1]: training_setup with opt.abs_grad, or the
                                                # first add_densification_stats(..., viewspace_abs=), creates it
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0
        self.grow_dir = grow_dir
        self.continous_dir = continous_dir
        self.grow_distance = grow_distance
        self.num_dirs = num_dirs
        self.modelcg = modelcg
        self.learn_split_distance = bool(getattr(modelcg, "learn_split_distance", False))
        self.learn_split_scale = bool(getattr(modelcg, "learn_split_scale", False))
        if self.grow_dir:                                       # :68-73 (an `elif` there: grow_dir wins)
            self._dirs_prob = torch.empty(0)
            self.dirs = torch.tensor(sphere_points(self.num_dirs)).to(torch.float32)      # moved with the parameters
        elif self.continous_dir:
            self._conti_dirs = torch.empty(0)
        if self.grow_distance:
            self._grow_dist = torch.empty(0)
        if self.learn_split_distance:
            self._split_distance = torch.empty(0)
        if self.learn_split_scale:
            self._split_scale = torch.empty(0)
        self._optimizer_cls = None                                   # None: the class opt.optimizer_type names
        # per-image exposure compensation (upstream 3DGS; setup_exposures): absent until asked for
        self._exposure = None
        self.exposure_mapping = {}
        self.pretrained_exposures = None
        self.exposure_optimizer = None
        # Mip-Splatting's 3D smoothing filter (filter3d.py): absent until compute_3D_filter is called
        self.filter_3D = None
        self.filter_3D_none_seen = None         # device int32 [1]: 1 when the cameras saw no Gaussian (the filter is 0)
        self._filter_3D_stale = False           # set by every operation that removes, adds, moves or permutes rows
        # :34-42; render's raw-parameter path recognises the model by these three
        self.scaling_activation = torch.exp
        self.scaling_inverse_activation = torch.log
        self.covariance_activation = covariance_from_scaling_rotation
        self.opacity_activation = torch.sigmoid
        self.inverse_opacity_activation = inverse_sigmoid
        self.rotation_activation = torch.nn.functional.normalize

    # ---- getters :151-194 -------------------------------------------------------------------------------------------
    @property
    def get_scaling(self):
        return self.scaling_activation(self._scaling)

    @property
    def get_grow_dist(self):
        return 2 * torch.sigmoid(self._grow_dist)

    @property
    def get_split_distance(self):
        return 2.2 * torch.sigmoid(self._split_distance)

    @property
    def get_split_scale(self):
        return 0.6 * torch.sigmoid(self._split_scale) + 0.5

    @property
    def get_rotation(self):
        return self.rotation_activation(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return self.opacity_activation(self._opacity)

    @property
    def get_dirs_prob(self):
        return self._dirs_prob

    @property
    def get_conti_dirs(self):
        return self._conti_dirs

    # ---- the 3D smoothing filter (Mip-Splatting's scene/gaussian_model.py; filter3d.py) --------------------------------
    @torch.no_grad()
    def compute_3D_filter(self, cameras, **kw):
        """``filter_3D [P]`` from the training cameras: ``filter3d.compute_3d_filter(self._xyz, cameras, **kw)`` (``near``,
        ``margin``, ``variance``, ``rule``).  From then on ``render`` draws the filtered model, until
        ``fuse_filter_3D_()`` bakes it in or ``filter_3D`` is set to None.  Call it again after every change of the rows
        (densification, pruning, reordering, MCMC relocation): those mark the filter stale and ``render`` refuses it."""
        _need_gpu("compute_3D_filter", self._xyz)
        self.filter_3D, self.filter_3D_none_seen = filter3d.compute_3d_filter(self._xyz.detach(), cameras, **kw)
        self._filter_3D_stale = False
        return self.filter_3D

    def checked_filter_3D(self, what: str = "render"):
        """``filter_3D``, or None for a model without one; ``ValueError`` for a stale or wrongly sized filter.  Host code."""
        return checked_filter_3D(self, what)

    @property
    def get_scaling_with_3D_filter(self):
        """``sqrt(exp(2 s) + f^2)`` ``[P,3]``; ``ValueError`` without a valid filter."""
        return filter3d.filtered_scaling_opacity(self._scaling, self._opacity, _required_filter(self, "get_scaling_with_3D_filter"))[0]

    @property
    def get_opacity_with_3D_filter(self):
        """``sigmoid(o) sqrt(prod a_i / prod (a_i + f^2))`` ``[P,1]``; ``ValueError`` without a valid filter."""
        return filter3d.filtered_scaling_opacity(self._scaling, self._opacity, _required_filter(self, "get_opacity_with_3D_filter"))[1]

    @torch.no_grad()
    def fuse_filter_3D_(self):
        """Bakes the filter into ``_scaling`` and ``_opacity`` in place (the effective raw values of
        ``filter3d.apply_3d_filter``; the ``Parameter`` objects and the optimizer's state stay) and drops it: the model
        then renders the same frames without a filter, in any viewer.  Nothing happens without a filter."""
        f = checked_filter_3D(self, "fuse_filter_3D_")
        if f is None:
            return self
        s, o = filter3d.apply_3d_filter(self._scaling.detach(), self._opacity.detach(), f)
        self._scaling.detach().copy_(s)
        self._opacity.detach().copy_(o)
        self.filter_3D = self.filter_3D_none_seen = None
        self._filter_3D_stale = False
        return self

    def get_covariance(self, scaling_modifier=1):
        return self.covariance_activation(self.get_scaling, scaling_modifier, self._rotation)

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ---- the tensors a model of these flags owns ------------------------------------------------------------------
    def _fork_attrs(self):
        """group name -> attribute of the fork tensors this model carries (``densify.FORK_FLAG``; ``:68-80``)."""
        return {k: a for k, a in FORK_ATTR.items() if getattr(self, FORK_FLAG[k], False) and hasattr(self, a)}

    def parameters(self):
        return [getattr(self, a) for a in list(GROUP_ATTR.values()) + list(self._fork_attrs().values())]

    # ---- initialisation :200-238 ------------------------------------------------------------------------------------
    @torch.no_grad()
    def create_from_pcd(self, points, colors=None, spatial_lr_scale: float = 1.0, *, dir_noise=None, dist2=None,
                        device=None):
        """``create_from_pcd(pcd, spatial_lr_scale)``.  points / colors: ``[N, 3]`` arrays or tensors (colours in
        [0, 1]), or one object with ``.points`` / ``.colors`` in place of both.  A tensor must already live on the GPU;
        arrays are moved to ``device`` (default: the current ROCm device).
        dir_noise: the ``[N, 3]`` standard-normal draws of ``:227`` (``continous_dir``; default ``torch.randn``).
        dist2: the ``[N]`` result of ``distCUDA2`` if the caller already has it (default: ``knn.distCUDA2``)."""
        if hasattr(points, "points") and hasattr(points, "colors"):      # create_from_pcd(pcd, spatial_lr_scale)
            if colors is not None:
                spatial_lr_scale = colors
            points, colors = points.points, points.colors
        if colors is None:
            raise TypeError("create_from_pcd needs points and colors")

        def on_device(a, name):
            if isinstance(a, torch.Tensor):
                _need_gpu("create_from_pcd", a)
                return a.detach().float()
            dev = torch.device(device if device is not None else "cuda")
            if dev.type != "cuda" or not torch.cuda.is_available():
                raise _lib.GsrError("create_from_pcd needs a ROCm GPU (no CPU path)")
            return torch.tensor(np.asarray(a)).float().to(dev)

        xyz = on_device(points, "points").contiguous()
        rgb = on_device(colors, "colors").to(xyz.device)
        if xyz.dim() != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape:
            raise ValueError(f"points and colors must both be [N, 3], got {tuple(xyz.shape)} and {tuple(rgb.shape)}")
        dev, N = xyz.device, int(xyz.shape[0])
        M = (self.max_sh_degree + 1) ** 2
        self.spatial_lr_scale = spatial_lr_scale
        f_dc = RGB2SH(rgb).reshape(N, 1, 3).contiguous()                              # :203-206, :218
        f_rest = torch.zeros((N, M - 1, 3), dtype=torch.float32, device=dev)          # :219
        if dist2 is None:
            dist2 = knn.distCUDA2(xyz)
        else:
            dist2 = torch.as_tensor(dist2, dtype=torch.float32).to(dev)
            if tuple(dist2.shape) != (N,):
                raise ValueError(f"dist2 must be [{N}], got {tuple(dist2.shape)}")
        dist2 = torch.clamp_min(dist2, MIN_DIST2)                                     # :210
        scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)                 # :211
        rots = torch.zeros((N, 4), dtype=torch.float32, device=dev)                   # :212-213
        rots[:, 0] = 1
        opacities = inverse_sigmoid(INITIAL_OPACITY * torch.ones((N, 1), dtype=torch.float32, device=dev))   # :215

        def param(t):
            return nn.Parameter(t.contiguous().requires_grad_(True))

        self._xyz = param(xyz.clone())
        self._features_dc = param(f_dc)
        self._features_rest = param(f_rest)
        self._scaling = param(scales)
        self._rotation = param(rots)
        self._opacity = param(opacities)
        if self.grow_dir:                                                             # :223-225
            self._dirs_prob = param(torch.ones((N, self.num_dirs), dtype=torch.float32, device=dev) / self.num_dirs)
            self.dirs = self.dirs.to(dev)
        if self.continous_dir:                                                        # :226-228
            if dir_noise is None:
                dir_noise = torch.randn((N, 3), dtype=torch.float32, device=dev)
            dir_noise = torch.as_tensor(dir_noise, dtype=torch.float32).to(dev)
            if tuple(dir_noise.shape) != (N, 3):
                raise ValueError(f"dir_noise must be [{N}, 3], got {tuple(dir_noise.shape)}")
            self._conti_dirs = param(torch.nn.functional.normalize(dir_noise, p=2.0, dim=-1))
        if self.grow_distance:                                                        # :229-231
            self._grow_dist = param(torch.zeros((N, 1), dtype=torch.float32, device=dev))
        if self.learn_split_distance:                                                 # :232-234
            self._split_distance = param(torch.zeros((N, 3), dtype=torch.float32, device=dev))
        if self.learn_split_scale:                                                    # :235-237
            self._split_scale = param(torch.zeros((N, 1), dtype=torch.float32, device=dev))
        self.max_radii2D = torch.zeros((N,), dtype=torch.float32, device=dev)         # :238
        return self

    # ---- per-image exposures (upstream 3DGS's gaussian_model.py; exposure.py) -----------------------------------------
    def setup_exposures(self, image_names, device=None):
        """One learnable 3x4 colour affine per training image, at the identity: ``_exposure`` ``[N,3,4]``,
        ``exposure_mapping`` name -> row, ``pretrained_exposures = None``.  Call it before ``training_setup``, which
        then builds ``exposure_optimizer``.  device: default where the model lives, else the current ROCm device (a
        CPU device is accepted: the tensor is host data until ``apply_exposure`` reads it)."""
        names = list(image_names)
        if not names:
            raise ValueError("setup_exposures needs at least one image name")
        if len(set(names)) != len(names):
            raise ValueError("setup_exposures needs distinct image names")
        if device is None:
            device = self._xyz.device if self._xyz.is_cuda else "cuda"
        eye = torch.eye(3, 4, dtype=torch.float32, device=device)
        self._exposure = nn.Parameter(eye[None].repeat(len(names), 1, 1).contiguous().requires_grad_(True))
        self.exposure_mapping = {name: i for i, name in enumerate(names)}
        self.pretrained_exposures = None
        self.exposure_optimizer = None
        return self

    @property
    def has_exposures(self) -> bool:
        return self._exposure is not None

    def get_exposure_from_name(self, image_name):
        """The ``[3,4]`` exposure of one image: a view of its row of ``_exposure`` (the gradient lands there), or the
        loaded tensor when ``pretrained_exposures`` is set.  ``KeyError`` for a name that has none."""
        table = self.exposure_mapping if self.pretrained_exposures is None else self.pretrained_exposures
        if image_name not in table:
            raise KeyError(f"no exposure for image {image_name!r}" +
                           ("" if table else " (setup_exposures has not been called and none were loaded)"))
        if self.pretrained_exposures is not None:
            return self.pretrained_exposures[image_name]
        return self._exposure[self.exposure_mapping[image_name]]

    # ---- optimizer :240-277 (optim.py) ------------------------------------------------------------------------------
    def training_setup(self, training_args, optimizer_cls=None):
        """optimizer_cls: None takes the class ``training_args.optimizer_type`` names (``optim.Adam`` by default)."""
        self._optimizer_cls = optimizer_cls
        return optim.training_setup(self, training_args, optimizer_cls)

    def update_learning_rate(self, iteration):
        return optim.update_learning_rate(self, iteration)

    # ---- reset_opacity :312-315 with replace_tensor_to_optimizer :386-399 -------------------------------------------
    @torch.no_grad()
    def reset_opacity(self):
        """Cap the opacities at 0.01 and zero the opacity group's Adam moments, in place, in one launch
        (``gsr_reset_opacity``): ``_opacity`` stays the same ``Parameter``.  What the reference's version does besides the
        values is kept: the state's ``step`` count stays, and ``_opacity.grad`` becomes None -- the reference builds a new
        ``Parameter`` and resets before ``optimizer.step()`` (``train.py:136-141``), so that iteration's step skips the
        opacity group."""
        p = self._opacity
        _need_gpu("reset_opacity", p)
        if p.dtype != torch.float32 or not p.is_contiguous():
            raise TypeError("reset_opacity needs a contiguous float32 _opacity")
        state = self.optimizer.state.get(p, None) if self.optimizer is not None else None
        moments = [state.get(k) if state else None for k in ("exp_avg", "exp_avg_sq")]
        for m in moments:
            if m is not None and not (m.is_cuda and m.device == p.device and m.dtype == torch.float32
                                      and m.is_contiguous() and m.numel() == p.numel()):
                raise TypeError("the opacity group's Adam moments must be contiguous float32 tensors like _opacity")
        with torch.cuda.device(p.device):
            stream = torch.cuda.current_stream(p.device).cuda_stream
            _lib.check(_lib.load().gsr_reset_opacity(p.data_ptr(), p.numel(), RESET_OPACITY_CAP,
                                                     *(m.data_ptr() if m is not None else None for m in moments),
                                                     stream), "gsr_reset_opacity")
        p.grad = None

    # ---- checkpoints :84-149 ----------------------------------------------------------------------------------------
    def capture(self):
        """The reference's 12-tuple of a plain model (``:118-131``).  A model with a fork flag appends a 13th element,
        the dict of its learned tensors by attribute name (this build's extension: the reference's own tuples for those
        models leave the optimizer state out and cannot be restored)."""
        out = (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
               self._opacity, self.max_radii2D, self.xyz_gradient_accum, self.denom, self.optimizer.state_dict(),
               self.spatial_lr_scale)
        fork = {a: getattr(self, a) for a in self._fork_attrs().values()}
        out = out + (fork,) if fork else out
        if self.has_exposures:                        # last, and told from the fork's dict by its "exposure_mapping" key
            out = out + ({"exposure": self._exposure, "exposure_mapping": dict(self.exposure_mapping),
                          "exposure_optimizer": self.exposure_optimizer.state_dict()},)
        if self.xyz_gradient_accum_abs is not None:   # behind everything else, and only when it exists: a model without
            out = out + ({"xyz_gradient_accum_abs": self.xyz_gradient_accum_abs},)      # it writes the tuples above
        if self.filter_3D is not None:                # last of all, and only when it exists
            out = out + ({"filter_3D": self.filter_3D, "filter_3D_stale": bool(self._filter_3D_stale)},)
        return out

    def restore(self, model_args, training_args, optimizer_cls=None):
        """``:133-149``; accepts every form ``capture`` returns: the 12-tuple, with the fork's dict, and either with the
        exposures' dict, and any of them with the absolute-gradient accumulator's dict, and any of those with the 3D
        filter's dict last (``ValueError`` when the checkpoint has exposures and this model none, or the reverse: call
        ``setup_exposures`` first, or not at all).  ``training_setup`` runs first, with
        ``optimizer_cls`` (default: the class ``training_setup`` was last given, else the one
        ``training_args.optimizer_type`` names: ``optim.Adam`` unless it says ``"sparse_adam"``), then the saved
        state is loaded into it: state dicts move freely between ``torch.optim.Adam`` and ``optim.Adam``."""
        model_args = tuple(model_args)
        filter_dict = None
        if model_args and isinstance(model_args[-1], dict) and "filter_3D" in model_args[-1]:
            filter_dict, model_args = model_args[-1], model_args[:-1]
        accum_abs = None
        if model_args and isinstance(model_args[-1], dict) and set(model_args[-1]) == {"xyz_gradient_accum_abs"}:
            accum_abs, model_args = model_args[-1]["xyz_gradient_accum_abs"], model_args[:-1]
        exposures = None
        if len(model_args) in (13, 14) and isinstance(model_args[-1], dict) and "exposure_mapping" in model_args[-1]:
            exposures, model_args = model_args[-1], model_args[:-1]
        if len(model_args) not in (12, 13):
            raise ValueError(f"restore expects the 12- or 13-element tuple of capture(), with the exposures' dict behind "
                             f"it for a model that has them, got {len(model_args) + (exposures is not None) + (accum_abs is not None)} "
                             f"elements")
        if (exposures is not None) != self.has_exposures:
            raise ValueError("the checkpoint holds exposures and this model has none (call setup_exposures before restore)"
                             if exposures is not None else
                             "this model has exposures and the checkpoint holds none")
        fork = model_args[12] if len(model_args) == 13 else {}
        want = set(self._fork_attrs().values())
        if not isinstance(fork, dict) or set(fork) != want:
            raise ValueError(f"the checkpoint holds the learned tensors {sorted(fork) if isinstance(fork, dict) else fork!r}, "
                             f"this model's flags need {sorted(want)}")
        (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
         self._opacity, self.max_radii2D, xyz_gradient_accum, denom, opt_dict, self.spatial_lr_scale) = model_args[:12]
        for a, t in fork.items():
            setattr(self, a, t)
        if self.grow_dir:
            self.dirs = self.dirs.to(self._xyz.device)
        if exposures is not None:
            self._exposure = exposures["exposure"]
            self.exposure_mapping = dict(exposures["exposure_mapping"])
        self.training_setup(training_args, optimizer_cls or self._optimizer_cls)
        self.xyz_gradient_accum = xyz_gradient_accum
        self.denom = denom
        if accum_abs is not None:                     # a checkpoint without it leaves what training_setup made
            self.xyz_gradient_accum_abs = accum_abs
        self.optimizer.load_state_dict(opt_dict)
        if exposures is not None:
            self.exposure_optimizer.load_state_dict(exposures["exposure_optimizer"])
        # a checkpoint without the filter's dict restores a model without a filter
        self.filter_3D = None if filter_dict is None else filter_dict["filter_3D"]
        self.filter_3D_none_seen = None
        self._filter_3D_stale = bool(filter_dict.get("filter_3D_stale", False)) if filter_dict is not None else False

    # ---- PLY :293-358 (ply_io.py) -----------------------------------------------------------------------------------
    def save_ply(self, path, fuse_filter=False):
        """``save_ply``.  A model that carries a 3D filter writes it as one more property, ``filter_3D``, behind ``rot_3``
        (Mip-Splatting's layout); a model without one writes the bytes it always wrote.  ``fuse_filter=True``: a standard
        PLY with the filter baked into ``scale_*`` and ``opacity`` (the effective raw values) and no ``filter_3D``
        property -- Mip-Splatting's fused PLY, for viewers that know nothing of the filter; the model itself is left as
        it is."""
        f = checked_filter_3D(self, "save_ply")
        if f is None:
            ply_io.save_ply(self, path)
        elif fuse_filter:
            with torch.no_grad():
                s, o = filter3d.apply_3d_filter(self._scaling.detach(), self._opacity.detach(), f)
            ply_io.save_ply(_Fused(self, s, o), path)
        else:
            ply_io.save_ply(self, path, filter_3D=f)

    def load_ply(self, path, device=None):
        """``load_ply``: the six parameters from the file, on ``device`` (default: where the model lives, else the
        current ROCm device); ``active_sh_degree`` becomes ``max_sh_degree`` (``:358``)."""
        if device is None:
            device = self._xyz.device if self._xyz.is_cuda else "cuda"
        if torch.device(device).type != "cuda" or not torch.cuda.is_available():
            raise _lib.GsrError("load_ply needs a ROCm GPU (no CPU path)")
        tensors = ply_io.load_ply(path, self.max_sh_degree, device)
        for a in GROUP_ATTR.values():
            setattr(self, a, nn.Parameter(tensors[a].requires_grad_(True)))
        self.active_sh_degree = self.max_sh_degree
        self.filter_3D = tensors.get("filter_3D")          # the file's, or None: a standard PLY carries no filter
        self.filter_3D_none_seen = None
        self._filter_3D_stale = False

    # ---- vector-quantised file (compress.py) -----------------------------------------------------------
    def save_compressed(self, path, **kw):
        """``compress.compress_model(self, **kw)`` written to ``path`` (one ``.npz``); returns the container."""
        from . import compress
        cg = compress.compress_model(self, **kw)
        compress.save_compressed(path, cg)
        return cg

    def load_compressed(self, path, device=None):
        """``load_ply`` for the file ``save_compressed`` writes: the six decoded parameters on ``device``."""
        from . import compress
        if device is None:
            device = self._xyz.device if self._xyz.is_cuda else "cuda"
        if torch.device(device).type != "cuda" or not torch.cuda.is_available():
            raise _lib.GsrError("load_compressed needs a ROCm GPU (no CPU path)")
        cg = compress.load_compressed(path)
        if cg.sh_degree != self.max_sh_degree:
            raise ValueError(f"{path}: SH degree {cg.sh_degree} does not match the model's {self.max_sh_degree}")
        tensors = cg.decode(device)
        for a in GROUP_ATTR.values():
            setattr(self, a, nn.Parameter(tensors[a].requires_grad_(True)))
        self.active_sh_degree = self.max_sh_degree
        self.filter_3D = self.filter_3D_none_seen = None
        self._filter_3D_stale = False


__all__ = ["GaussianModel", "sphere_points", "inverse_sigmoid", "checked_filter_3D"]
