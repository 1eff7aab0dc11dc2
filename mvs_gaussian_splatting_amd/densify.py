"""Densification bookkeeping on the HIP path: ``GaussianModel.densify_and_prune``
(``scene/gaussian_model.py:750-772``, plain branch) with its clone (``:580-610``), split (``:506-578``), postfix
(``:466-504``) and prune (``:401-449``) steps, including the Adam-moment surgery of ``_prune_optimizer`` /
``cat_tensors_to_optimizer`` (``:401-422``, ``:451-472``).

One plan kernel classifies every Gaussian, then every parameter / moment tensor is read once and written once
(``gsr_densify_*``); the reference's ~60 boolean-index / cat / repeat launches (a host sync each) are gone.  The
result is the reference's, row for row: ``[kept originals | clones | first children | second children]``.

The model is duck-typed on the reference's attributes: ``_xyz, _features_dc, _features_rest, _opacity, _scaling,
_rotation, xyz_gradient_accum, denom, max_radii2D, percent_dense`` and, optionally, ``optimizer`` (``torch.optim.Adam``
whose param groups are named ``xyz, f_dc, f_rest, opacity, scaling, rotation`` -- ``training_setup``, ``:240-252``).
There is no CPU path.

The fork's models (``grow_dir`` / ``continous_dir`` / ``grow_distance`` / ``learn_split_distance`` /
``learn_split_scale``) take ``csrc/densify_fork.hip``: the same plan / gather shape over their learned tensors
(``_dirs_prob, _conti_dirs, _grow_dist, _split_distance, _split_scale`` and the optimizer groups of the same names,
``:253-262``), and the grow branch of ``:755`` (``densify_and_grow`` :612-677 + ``densify_and_growsplit`` :679-749) with
its re-inits.  ``branch()`` says which branch a call takes.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch
from torch import nn

from . import _lib

GROUP_ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
              "scaling": "_scaling", "rotation": "_rotation"}
# the fork's learned tensors: optimizer group -> attribute, and the model flag that creates it (:64-79, :253-262)
FORK_ATTR = {"dirs_prob": "_dirs_prob", "conti_dirs": "_conti_dirs", "grow_dist": "_grow_dist",
             "split_distance": "_split_distance", "split_scale": "_split_scale"}
FORK_FLAG = {"dirs_prob": "grow_dir", "conti_dirs": "continous_dir", "grow_dist": "grow_distance",
             "split_distance": "learn_split_distance", "split_scale": "learn_split_scale"}
GROW, CLONE_SPLIT = "grow", "clone_split"


def mark_filter_stale(model) -> None:
    """Every package operation that removes, adds, moves or permutes rows calls this: a ``filter_3D`` computed for the old
    rows must be recomputed (``GaussianModel.compute_3D_filter``) before ``render`` accepts the model again.  A model
    without a filter is left exactly as it is."""
    if getattr(model, "filter_3D", None) is not None:
        model._filter_3D_stale = True


def swap_rows_(model, attrs, new, moment) -> None:
    """The optimizer surgery every change of the row count shares (``_prune_optimizer`` / ``cat_tensors_to_optimizer``,
    ``:401-422``, ``:451-472``).  ``attrs``: ``{group name: model attribute}``; ``new``: ``{group name: new tensor}``;
    ``moment``: maps an old ``exp_avg`` / ``exp_avg_sq`` tensor to the new one.

    Every group of ``model.optimizer`` (if any) named in ``new`` gets a fresh ``nn.Parameter`` over the new tensor.  The
    state dict of the old parameter always moves to the new one, whatever it holds: ``exp_avg`` and ``exp_avg_sq`` go
    through ``moment`` where present, every other key (``step`` included) is carried over as it is, and no entry stays
    behind under the dead parameter.  A tensor that no group owns keeps its kind (``nn.Parameter`` or plain tensor) and
    its ``requires_grad``.  The model's attributes are then set.  A model that carries a 3D smoothing filter
    (``filter_3D``; filter3d.py) has it marked stale: its rows no longer belong to these rows."""
    mark_filter_stale(model)
    optimizer = getattr(model, "optimizer", None)
    owned = {}
    for group in optimizer.param_groups if optimizer is not None else ():
        name = group.get("name")
        if name not in new:
            continue
        old = group["params"][0]
        owned[name] = group["params"][0] = nn.Parameter(new[name].requires_grad_(True))
        stored = optimizer.state.pop(old, None)
        if stored is not None:
            for key in ("exp_avg", "exp_avg_sq"):
                if key in stored:
                    stored[key] = moment(stored[key])
            optimizer.state[owned[name]] = stored
    for k, a in attrs.items():
        t, old = owned.get(k), getattr(model, a)
        if t is None:
            t = nn.Parameter(new[k], requires_grad=old.requires_grad) if isinstance(old, nn.Parameter) \
                else new[k].requires_grad_(old.requires_grad)
        setattr(model, a, t)


def _gather(call, name, P, src, n_out):
    """``call(row floats, src pointer, dst pointer)`` -- a ``gsr_densify_*gather_rows`` -- over one ``[P, ...]`` tensor
    -> ``[n_out, ...]``.  A tensor without rows or without width (``_features_rest`` ``[P,0,3]`` at degree 0) has
    nothing to gather: the library refuses ``row_floats <= 0``."""
    src = src.detach().contiguous()
    w = src.numel() // max(P, 1)
    dst = torch.empty((n_out,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    if P > 0 and w > 0:
        _lib.check(call(w, src.data_ptr(), dst.data_ptr()), name)
    return dst


def _reset_stats(model, n_out, dev) -> None:
    model.xyz_gradient_accum = torch.zeros((n_out, 1), dtype=torch.float32, device=dev)      # :501-503
    model.denom = torch.zeros((n_out, 1), dtype=torch.float32, device=dev)
    model.max_radii2D = torch.zeros((n_out,), dtype=torch.float32, device=dev)


def _flag(obj, name) -> bool:
    return bool(getattr(obj, name, False))


def fork_flags(model) -> Dict[str, bool]:
    """The fork's switches of a model: the five tensor flags plus ``modelcg.{symmetric_split, split_notreinit,
    prob_notreinit}``.  All False for a plain model."""
    cg = getattr(model, "modelcg", None)
    out = {f: _flag(model, f) for f in FORK_FLAG.values()}
    out.update({f: _flag(cg, f) for f in ("symmetric_split", "split_notreinit", "prob_notreinit")})
    return out


def is_fork(model) -> bool:
    """True when ``densify_and_prune`` takes the fork's path: a tensor flag is set, or a learned tensor is present."""
    return any(_flag(model, f) for f in FORK_FLAG.values()) or any(
        isinstance(getattr(model, a, None), torch.Tensor) and getattr(model, a).numel() > 0 for a in FORK_ATTR.values())


def branch(model, opt=None, iteration=None) -> str:
    """Which branch ``densify_and_prune`` runs (``:755``): ``"grow"`` when ``grow_dir`` or ``continous_dir`` is set and
    ``iteration > opt.opacity_reset_interval``, else ``"clone_split"``.  Host-only: reads Python values, never a
    tensor.  A grow model needs ``opt`` and ``iteration`` (the reference compares them unconditionally)."""
    if not (_flag(model, "grow_dir") or _flag(model, "continous_dir")):
        return CLONE_SPLIT
    if opt is None or iteration is None:
        raise ValueError("a grow_dir / continous_dir model needs opt and iteration to choose its densification branch "
                         "(scene/gaussian_model.py:755)")
    return GROW if iteration > opt.opacity_reset_interval else CLONE_SPLIT


@torch.no_grad()
def densify_and_prune(model, max_grad: float, min_opacity: float, extent: float, max_screen_size,
                      noise: Optional[torch.Tensor] = None, spatial_order: bool = False, *, opt=None, iteration=None,
                      dir_noise: Optional[torch.Tensor] = None, abs_grad_threshold: Optional[float] = None) -> Dict[str, int]:
    """In-place equivalent of ``gaussians.densify_and_prune(max_grad, min_opacity, extent, max_screen_size)``
    (``train.py:134``).  ``noise`` (``[2 * n_split_selected, 3]`` standard normal; default: ``torch.randn`` on the
    device) stands for the draws of ``torch.normal(mean=0, std=stds)`` at ``:537-539``.  ``spatial_order`` (this build's
    extension, off by default): store the result along a Morton curve instead of the reference's ``[kept | clones |
    children]`` row order (``layout.reorder_gaussians_``: the same Gaussians and moments, permuted; the frames that follow
    are 6-9 % faster at 6 M Gaussians).

    A fork model (``is_fork``) densifies as ``gaussians.densify_and_prune(..., opt, iteration)`` does
    (``train.py:134``): ``branch(model, opt, iteration)`` picks the grow or the clone + split branch; ``noise`` holds the
    split's standard-normal draws in the reference's order over its split rows (``[2n,3]``, ``[n,3]`` with
    ``symmetric_split``, ``[0,3]`` with ``learn_split_distance``) and ``dir_noise`` (``[selected,3]``) the
    ``torch.randn`` of the continuous re-init (``:650``); both default to fresh draws.  The returned dict then also
    holds ``branch``, ``grown`` and ``selected``.

    ``abs_grad_threshold`` (AbsGS / PGSR's ``densify_abs_grad_threshold``; None: the call above, bit for bit): the plan also
    reads ``model.xyz_gradient_accum_abs`` (``losses.add_densification_stats(..., viewspace_abs=)``) and SPLITS a large
    Gaussian when ``grad >= max_grad`` or ``grad_abs >= abs_grad_threshold``; clone and prune are unchanged
    (``gsr_densify_plan_abs``, ``include/gsr.h``).  Not available for a fork model (``ValueError``)."""
    if abs_grad_threshold is not None:
        if is_fork(model):
            raise ValueError("abs_grad_threshold is not available for a grow / learned-split (fork) model: its plan has no "
                             "absolute-gradient rule")
        accum_abs = getattr(model, "xyz_gradient_accum_abs", None)
        if not isinstance(accum_abs, torch.Tensor) or accum_abs.numel() != int(model._xyz.shape[0]):
            raise ValueError("abs_grad_threshold needs model.xyz_gradient_accum_abs with one value per Gaussian "
                             "(add_densification_stats(..., viewspace_abs=) fills it)")
    if is_fork(model):
        return _densify_fork(model, max_grad, min_opacity, extent, max_screen_size, noise, spatial_order, opt,
                             iteration, dir_noise)
    lib = _lib.load()
    xyz = model._xyz
    if not xyz.is_cuda:
        raise _lib.GsrError("densify_and_prune needs ROCm GPU tensors (no CPU path)")
    dev = xyz.device
    P = int(xyz.shape[0])
    params = {k: getattr(model, a) for k, a in GROUP_ATTR.items()}
    for k, t in params.items():
        if t.dtype != torch.float32 or t.shape[0] != P:
            raise TypeError(f"{k}: expected float32 with {P} rows")
    accum = model.xyz_gradient_accum.detach().to(torch.float32).contiguous()
    denom = model.denom.detach().to(torch.float32).contiguous()
    ws = torch.empty(max(lib.gsr_densify_workspace_bytes(P), 256), dtype=torch.uint8, device=dev)
    counts = (C.c_uint32 * 4)()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        scaling = params["scaling"].detach().contiguous()
        opacity = params["opacity"].detach().contiguous()
        tail = (float(model.percent_dense * extent), float(min_opacity), float(0.1 * extent) if max_screen_size else -1.0,
                ws.data_ptr(), ws.numel(), counts, stream)
        if abs_grad_threshold is None:
            _lib.check(lib.gsr_densify_plan(P, accum.data_ptr(), denom.data_ptr(), scaling.data_ptr(), opacity.data_ptr(),
                                            float(max_grad), *tail), "gsr_densify_plan")
        else:
            accum_abs = model.xyz_gradient_accum_abs.detach().to(dev, torch.float32).contiguous()
            _lib.check(lib.gsr_densify_plan_abs(P, accum.data_ptr(), accum_abs.data_ptr(), denom.data_ptr(),
                                                scaling.data_ptr(), opacity.data_ptr(), float(max_grad),
                                                float(abs_grad_threshold), *tail), "gsr_densify_plan_abs")
        n_keep, n_clone, n_child, n_sel = (int(v) for v in counts)
        n_out = n_keep + n_clone + 2 * n_child
        if noise is None:
            noise = torch.randn(2 * n_sel, 3, dtype=torch.float32, device=dev)
        noise = noise.to(dev, torch.float32).contiguous()
        if tuple(noise.shape) != (2 * n_sel, 3):
            raise ValueError(f"noise must be [{2 * n_sel}, 3] (2 x split-selected), got {tuple(noise.shape)}")
        def rows(t, zero_new):
            return _gather(lambda w, src, dst: lib.gsr_densify_gather_rows(P, w, src, ws.data_ptr(), counts, zero_new, dst,
                                                                           stream), "gsr_densify_gather_rows", P, t, n_out)
        new = {k: rows(t, 0) for k, t in params.items()}
        _lib.check(lib.gsr_densify_split_children(P, params["xyz"].detach().contiguous().data_ptr(), scaling.data_ptr(),
                                                  params["rotation"].detach().contiguous().data_ptr(), noise.data_ptr(),
                                                  ws.data_ptr(), counts, new["xyz"].data_ptr(), new["scaling"].data_ptr(),
                                                  stream), "gsr_densify_split_children")
        swap_rows_(model, GROUP_ATTR, new, lambda m: rows(m, 1))          # new rows: zero moments (:458-459)
    _reset_stats(model, n_out, dev)
    if getattr(model, "xyz_gradient_accum_abs", None) is not None:
        model.xyz_gradient_accum_abs = torch.zeros((n_out, 1), dtype=torch.float32, device=dev)
    if spatial_order:
        from .layout import reorder_gaussians_
        reorder_gaussians_(model)
    return {"points": n_out, "kept": n_keep, "cloned": n_clone, "split_selected": n_sel, "children_per_copy": n_child}


def _fork_inputs(model, P):
    """The model's learned tensors by group name, checked against their flags."""
    flags = fork_flags(model)
    if flags["grow_dir"] and flags["continous_dir"]:
        raise ValueError("grow_dir and continous_dir are exclusive (the reference's densify_and_grow runs one of them, "
                         ":617-624, and its postfix then misses the other's tensor)")
    widths = {"conti_dirs": 3, "grow_dist": 1, "split_distance": 3, "split_scale": 1}
    if flags["grow_dir"]:
        nd = getattr(model, "num_dirs", None)
        dirs = getattr(model, "dirs", None)
        if not isinstance(nd, int) or nd <= 0:
            raise ValueError("grow_dir needs model.num_dirs > 0")
        if not isinstance(dirs, torch.Tensor) or tuple(dirs.shape) != (nd, 3):
            raise ValueError(f"grow_dir needs model.dirs of shape [{nd}, 3]")
        widths["dirs_prob"] = nd
    out = {}
    for name, attr in FORK_ATTR.items():
        t = getattr(model, attr, None)
        if not flags[FORK_FLAG[name]]:
            if isinstance(t, torch.Tensor) and t.dim() >= 1 and t.shape[0] == P and P > 0:
                raise ValueError(f"{attr} is present but {FORK_FLAG[name]} is off: the reference would leave it at the "
                                 "old row count")
            continue
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{FORK_FLAG[name]} is set but the model has no {attr}")
        if tuple(t.shape) != (P, widths[name]) or t.dtype != torch.float32 or t.device != model._xyz.device:
            raise ValueError(f"{attr}: expected float32 [{P}, {widths[name]}] on {model._xyz.device}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
        out[name] = t
    return flags, out


def _densify_fork(model, max_grad, min_opacity, extent, max_screen_size, noise, spatial_order, opt, iteration,
                  dir_noise):
    lib = _lib.load()
    xyz = model._xyz
    if not xyz.is_cuda:
        raise _lib.GsrError("densify_and_prune needs ROCm GPU tensors (no CPU path)")
    dev = xyz.device
    P = int(xyz.shape[0])
    params = {k: getattr(model, a) for k, a in GROUP_ATTR.items()}
    for k, t in params.items():
        if t.dtype != torch.float32 or t.shape[0] != P:
            raise TypeError(f"{k}: expected float32 with {P} rows")
    flags, learned = _fork_inputs(model, P)
    grow = branch(model, opt, iteration) == GROW
    reinit = grow and not flags["prob_notreinit"]
    mode = ((_lib.GROW_DIR if flags["grow_dir"] else 0) | (_lib.GROW_CONTINUOUS if flags["continous_dir"] else 0) |
            (_lib.GROW_DISTANCE if flags["grow_distance"] else 0) |
            (_lib.SPLIT_DISTANCE if flags["learn_split_distance"] else 0) |
            (_lib.SPLIT_SCALE if flags["learn_split_scale"] else 0) | (_lib.DENSIFY_GROW if grow else 0) |
            (_lib.DENSIFY_SYMMETRIC if flags["symmetric_split"] else 0))
    accum = model.xyz_gradient_accum.detach().to(torch.float32).contiguous()
    denom = model.denom.detach().to(torch.float32).contiguous()
    if accum.numel() != P or denom.numel() != P:
        raise ValueError("xyz_gradient_accum / denom need one value per Gaussian")
    ws = torch.empty(max(lib.gsr_densify_fork_workspace_bytes(P), 256), dtype=torch.uint8, device=dev)
    counts = (C.c_uint32 * 5)()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        src = {k: t.detach().contiguous() for k, t in params.items()}
        src.update({k: t.detach().contiguous() for k, t in learned.items()})
        split_scale = src.get("split_scale")
        _lib.check(lib.gsr_densify_fork_plan(P, accum.data_ptr(), denom.data_ptr(), src["scaling"].data_ptr(),
                                             src["opacity"].data_ptr(),
                                             split_scale.data_ptr() if split_scale is not None else None,
                                             float(max_grad), float(model.percent_dense * extent), float(min_opacity),
                                             float(0.1 * extent) if max_screen_size else -1.0, ws.data_ptr(),
                                             ws.numel(), counts, stream), "gsr_densify_fork_plan")
        n_orig, n_extra, n_child, n_split, n_sel = (int(v) for v in counts)
        n_out = n_orig + n_extra + (4 if grow else 2) * n_child
        n_a = 2 * n_split if grow else n_split                      # split rows of A (:693-695)
        if flags["learn_split_distance"]:
            want = (0, 3)
        elif flags["symmetric_split"]:
            want = (n_a, 3)
        else:
            want = (2 * n_a, 3)
        if noise is None:
            noise = torch.randn(want, dtype=torch.float32, device=dev)
        noise = noise.to(dev, torch.float32).contiguous()
        if tuple(noise.shape) != want:
            raise ValueError(f"noise must be {list(want)} (the split's draws over {n_a} split rows), got "
                             f"{list(noise.shape)}")
        conti_reinit = reinit and flags["continous_dir"]
        want_dir = (n_sel if conti_reinit else 0, 3)
        if dir_noise is None:
            dir_noise = torch.randn(want_dir, dtype=torch.float32, device=dev)
        dir_noise = dir_noise.to(dev, torch.float32).contiguous()
        if tuple(dir_noise.shape) != want_dir:
            raise ValueError(f"dir_noise must be {list(want_dir)} (the continuous re-init's draws, one per selected "
                             f"Gaussian), got {list(dir_noise.shape)}")

        cp, const, skip = _lib.ROW_COPY, _lib.ROW_CONST, _lib.ROW_SKIP
        policy = {k: (_lib.ROW_POLICY(cp, cp, cp), 0.0) for k in src}
        policy["xyz"] = (_lib.ROW_POLICY(cp, skip if grow else cp, skip), 0.0)
        policy["scaling"] = (_lib.ROW_POLICY(cp, cp, skip), 0.0)
        if reinit and "dirs_prob" in src:                                     # :646-648
            policy["dirs_prob"] = (_lib.ROW_POLICY(const, const, const),
                                   float(torch.tensor(1.0) / int(model.num_dirs)))
        if conti_reinit:                                                      # :650-651
            policy["conti_dirs"] = (_lib.ROW_POLICY(skip, skip, skip), 0.0)
        if reinit and "grow_dist" in src:                                     # :652-654
            policy["grow_dist"] = (_lib.ROW_POLICY(const, const, const), 0.0)
        if not flags["split_notreinit"]:                                      # :558-574 / :729-745
            for k in ("split_distance", "split_scale"):
                if k in src:
                    policy[k] = (_lib.ROW_POLICY(cp, cp, const), 0.0)
        def rows(t, pol, value):
            return _gather(lambda w, s, dst: lib.gsr_densify_fork_gather_rows(P, w, s, ws.data_ptr(), counts,
                                                                              1 if grow else 0, pol, float(value), dst,
                                                                              stream),
                           "gsr_densify_fork_gather_rows", P, t, n_out)
        new = {k: rows(t, *policy[k]) for k, t in src.items()}
        fk = _lib.GsrDensifyFork()
        fk.P, fk.mode = P, mode
        fk.num_dirs = int(model.num_dirs) if flags["grow_dir"] else 0
        dirs = model.dirs.detach().to(dev, torch.float32).contiguous() if flags["grow_dir"] else None
        ptr = lambda t: t.data_ptr() if t is not None else None       # noqa: E731
        fk.xyz, fk.scaling, fk.rotation = ptr(src["xyz"]), ptr(src["scaling"]), ptr(src["rotation"])
        fk.dirs_prob, fk.dirs, fk.conti_dirs = ptr(src.get("dirs_prob")), ptr(dirs), ptr(src.get("conti_dirs"))
        fk.grow_dist, fk.split_distance = ptr(src.get("grow_dist")), ptr(src.get("split_distance"))
        fk.split_scale, fk.noise, fk.dir_noise = ptr(split_scale), ptr(noise), ptr(dir_noise)
        _lib.check(lib.gsr_densify_fork_rows(C.byref(fk), ws.data_ptr(), counts, new["xyz"].data_ptr(),
                                             new["scaling"].data_ptr(),
                                             new["conti_dirs"].data_ptr() if conti_reinit else None, stream),
                   "gsr_densify_fork_rows")
        zero_new = _lib.ROW_POLICY(cp, const, const)                     # new rows: zero moments (:458-459)
        swap_rows_(model, dict(GROUP_ATTR, **{k: FORK_ATTR[k] for k in learned}), new,
                   lambda m: rows(m, zero_new, 0.0))
    _reset_stats(model, n_out, dev)
    if spatial_order:
        from .layout import reorder_gaussians_
        reorder_gaussians_(model)
    return {"points": n_out, "kept": n_orig, "cloned": 0 if grow else n_extra, "grown": n_extra if grow else 0,
            "split_selected": n_split, "children_per_copy": n_child, "selected": n_sel,
            "branch": GROW if grow else CLONE_SPLIT}
