"""The fork's grow / learned-split branch of ``render()`` (``gaussian_renderer/__init__.py:91-253``) on the HIP path.

While the branch is open, every training frame renders the model together with G "virtual" Gaussians appended after its
P rows (row ``P + j`` comes from source row ``src[j]``, sources in row order):

* grow mode (``grow_dir`` or ``continous_dir``, ``:94-119``): a copy of every Gaussian with ``|accum / denom| >= thr``,
  moved by ``dir * max(exp(scaling)) * d`` -- ``dir`` the straight-through one-hot of ``softmax(_dirs_prob)`` times
  ``dirs`` (``scene/gaussian_model.py:360-366``) or ``normalize(_conti_dirs)``; ``d = 2 sigmoid(_grow_dist)`` with
  ``grow_distance``, else 1;
* learned split (``learn_split_distance`` / ``learn_split_scale``, ``:186-253``): every selected Gaussian whose largest
  scale exceeds ``percent_dense * cameras_extent`` moves to ``xyz + R s`` and its copy sits at ``xyz - R s``, both with
  ``scaling / k``; ``s = exp(scaling) * 2.2 sigmoid(_split_distance)`` or a ``normal(0, exp(scaling))`` draw,
  ``k = 2 (0.6 sigmoid(_split_scale) + 0.5)`` or 1.6.

Three kernels of ``csrc/grow.hip`` do the work: a plan (selection + block scan, one count read-back), an expansion into
the extended raw-parameter tensors the fused rasterizer takes unchanged, and a fold of the virtual rows' gradients onto
their sources with the chain rule into the learned tensors.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from . import _lib

GROW, SPLIT = "grow", "split"

# the reference line that cannot run: grow mode with a learned split and at least one split row
# concatenates new_split_scales twice (:166/:175 and :181), so its assert at :185 fails
_QUIRK = ("the reference's grow + learned-split path cannot render this frame: with grow_dir / continous_dir and "
          "learn_split_distance / learn_split_scale, {n} rows qualify for the split, and "
          "gaussian_renderer/__init__.py:181 concatenates new_split_scales a second time, so the assert "
          "`scales.size(0) == means3D.size(0)` at :185 fails")


def _split_flags(modelcg):
    if modelcg is None:
        return False, False
    return bool(getattr(modelcg, "learn_split_distance", False)), bool(getattr(modelcg, "learn_split_scale", False))


def branch(iteration, opt, grow_dir=False, continous_dir=False, modelcg=None) -> Optional[str]:
    """Which branch of ``gaussian_renderer/__init__.py:91-186`` a frame takes: ``"grow"``, ``"split"`` or ``None`` (the
    plain frame).  Host-only: reads Python values, never a tensor."""
    if iteration is None or opt is None:
        return None
    learn_d, learn_s = _split_flags(modelcg)
    if (grow_dir or continous_dir) and iteration > (opt.densify_from_iter - opt.densification_interval - 1) and \
            iteration < opt.densify_until_iter:
        # :93: inside the window the branch acts only after the first opacity reset; the learned split is not tried
        return GROW if iteration > opt.opacity_reset_interval else None
    if learn_d or learn_s:
        return SPLIT
    return None


def mode_bits(which: str, grow_dir=False, continous_dir=False, grow_distance=False, modelcg=None) -> int:
    """GSR_GROW_* / GSR_SPLIT_* bits of a branch.  In grow mode the split flags only matter for the check of :185."""
    learn_d, learn_s = _split_flags(modelcg)
    if which == GROW:
        m = _lib.GROW_DIR if grow_dir else _lib.GROW_CONTINUOUS      # `if grow_dir: ... elif continous_dir:` (:98-103)
        return m | (_lib.GROW_DISTANCE if grow_distance else 0)
    return (_lib.SPLIT_DISTANCE if learn_d else 0) | (_lib.SPLIT_SCALE if learn_s else 0)


class Plan(NamedTuple):
    P: int
    G: int
    mode: int
    vidx: torch.Tensor        # int32 [P]: virtual row of each Gaussian, or -1
    src: torch.Tensor         # int32 [G]: source row of each virtual row
    selected: torch.Tensor    # bool [P]: the reference's selected_pts_mask
    n_big: int                # selected rows whose largest scale exceeds percent_dense * extent


def plan(pc, mode: int, densify_grad_threshold: float, percent_dense_extent: float) -> Plan:
    """Selection of the frame (``:94-96`` / ``:189-194``).  Synchronises the stream once, for G."""
    lib = _lib.load()
    xyz = pc._xyz
    dev = xyz.device
    P = int(xyz.shape[0])
    accum = pc.xyz_gradient_accum.detach().to(torch.float32).contiguous()
    denom = pc.denom.detach().to(torch.float32).contiguous()
    scaling = pc._scaling.detach().contiguous()
    if accum.numel() != P or denom.numel() != P or scaling.shape != (P, 3) or not accum.is_cuda:
        raise ValueError("xyz_gradient_accum / denom need one GPU value per Gaussian and _scaling [P,3]")
    with torch.cuda.device(dev):
        ws = torch.empty(max(lib.gsr_grow_workspace_bytes(P), 256), dtype=torch.uint8, device=dev)
        vidx = torch.empty(P, dtype=torch.int32, device=dev)
        src = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
        selected = torch.empty(P, dtype=torch.bool, device=dev)
        counts = (C.c_uint32 * 2)()
        _lib.check(lib.gsr_grow_plan(P, accum.data_ptr(), denom.data_ptr(), scaling.data_ptr(),
                                     float(densify_grad_threshold), float(percent_dense_extent), int(mode),
                                     ws.data_ptr(), ws.numel(), vidx.data_ptr(), src.data_ptr(), selected.data_ptr(),
                                     counts, torch.cuda.current_stream(dev).cuda_stream), "gsr_grow_plan")
    G = int(counts[0])
    return Plan(P, G, int(mode), vidx, src[:G], selected, int(counts[1]))


_LEARNED = ("dirs_prob", "conti_dirs", "grow_dist", "split_distance", "split_scale")


def _learned_for(mode: int):
    """Which learned tensors a mode reads (and differentiates)."""
    grow = mode & (_lib.GROW_DIR | _lib.GROW_CONTINUOUS)
    return {"dirs_prob": bool(mode & _lib.GROW_DIR), "conti_dirs": bool(mode & _lib.GROW_CONTINUOUS),
            "grow_dist": bool(grow and mode & _lib.GROW_DISTANCE),
            "split_distance": bool(not grow and mode & _lib.SPLIT_DISTANCE),
            "split_scale": bool(not grow and mode & _lib.SPLIT_SCALE)}


def _params(pl: Plan, xyz, f_dc, f_rest, opacity, scaling, rotation, learned, dirs, noise):
    g = _lib.GsrGrow()
    g.P, g.G, g.mode = pl.P, pl.G, pl.mode
    g.n_rest = int(f_rest.numel() // max(pl.P, 1))
    g.num_dirs = int(dirs.shape[0]) if dirs is not None else 0
    g.xyz, g.f_dc, g.opacity, g.scaling, g.rotation = (t.data_ptr() for t in (xyz, f_dc, opacity, scaling, rotation))
    g.f_rest = f_rest.data_ptr() if g.n_rest else None
    for k in _LEARNED:
        t = learned.get(k)
        setattr(g, k, t.data_ptr() if t is not None else None)
    g.dirs = dirs.data_ptr() if dirs is not None else None
    g.noise = noise.data_ptr() if noise is not None and noise.numel() else None
    g.vidx = pl.vidx.data_ptr()
    g.src = pl.src.data_ptr() if pl.G else None
    return g


def _c32(t, name, dev, shape=None):
    if t.device != dev or t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 on {dev}")
    t = t.detach().contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {list(shape)}, got {list(t.shape)}")
    return t


class _GrowExpand(torch.autograd.Function):
    """Raw model tensors (+ the learned tensors of the mode) -> the [P+G]-row raw tensors the fused rasterizer takes."""

    @staticmethod
    def forward(ctx, pl: Plan, dirs, noise, xyz, means2D, f_dc, f_rest, opacity, scaling, rotation, dirs_prob, conti_dirs,
                grow_dist, split_distance, split_scale):
        lib = _lib.load()
        dev = xyz.device
        P, G = pl.P, pl.G
        xyz = _c32(xyz, "xyz", dev, (P, 3))
        f_dc = _c32(f_dc, "f_dc", dev)
        f_rest = _c32(f_rest, "f_rest", dev)
        opacity = _c32(opacity, "opacity", dev, (P, 1))
        scaling = _c32(scaling, "scaling", dev, (P, 3))
        rotation = _c32(rotation, "rotation", dev, (P, 4))
        if f_dc.numel() != 3 * P or f_rest.numel() not in (0, 45 * P):
            raise ValueError("f_dc must be [P,1,3] and f_rest [P,15,3] or [P,0,3]")
        use = _learned_for(pl.mode)
        given = dict(zip(_LEARNED, (dirs_prob, conti_dirs, grow_dist, split_distance, split_scale)))
        width = {"conti_dirs": 3, "grow_dist": 1, "split_distance": 3, "split_scale": 1}
        learned = {}
        for k in _LEARNED:
            if use[k]:
                if given[k] is None:
                    raise ValueError(f"the branch needs the model's _{k}")
                shape = (P, int(dirs.shape[0])) if k == "dirs_prob" else (P, width[k])
                learned[k] = _c32(given[k], "_" + k, dev, shape)
        if use["dirs_prob"]:
            dirs = _c32(dirs, "dirs", dev, (learned["dirs_prob"].shape[1], 3))
        else:
            dirs = None
        if noise is not None:
            noise = _c32(noise, "noise", dev, (G, 3))
        new = lambda like: torch.empty((P + G,) + tuple(like.shape[1:]), dtype=torch.float32, device=dev)  # noqa: E731
        outs = [new(t) for t in (xyz, f_dc, f_rest, opacity, scaling, rotation)]
        g = _params(pl, xyz, f_dc, f_rest, opacity, scaling, rotation, learned, dirs, noise)
        with torch.cuda.device(dev):
            _lib.check(lib.gsr_grow_expand(C.byref(g), *(o.data_ptr() if o.numel() else None for o in outs),
                                           torch.cuda.current_stream(dev).cuda_stream), "gsr_grow_expand")
        # means2D: the operator never reads its values, only its gradient leaves -- an uninitialised [P+G,3] block
        m2 = torch.empty(P + G, 3, dtype=torch.float32, device=dev)
        ctx.pl, ctx.keep = pl, (dirs, noise)
        ctx.learned_keys = [k for k in _LEARNED if k in learned]
        ctx.save_for_backward(xyz, f_dc, f_rest, opacity, scaling, rotation, *(learned[k] for k in ctx.learned_keys))
        ctx.shapes = (tuple(means2D.shape), tuple(f_dc.shape), tuple(f_rest.shape))
        return outs[0], m2, outs[1], outs[2], outs[3], outs[4], outs[5]

    @staticmethod
    def backward(ctx, g_xyz, g_m2, g_dc, g_rest, g_op, g_sc, g_rot):
        lib = _lib.load()
        pl = ctx.pl
        xyz, f_dc, f_rest, opacity, scaling, rotation, *lt = ctx.saved_tensors
        learned = dict(zip(ctx.learned_keys, lt))
        dirs, noise = ctx.keep
        dev = xyz.device
        P = pl.P
        gin = [t.to(torch.float32).contiguous() for t in (g_xyz, g_m2, g_dc, g_rest, g_op, g_sc, g_rot)]
        shapes = [(P, 3), ctx.shapes[0], ctx.shapes[1], ctx.shapes[2], (P, 1), (P, 3), (P, 4)]
        gout = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
        dl = {}
        for k, t in learned.items():
            dl[k] = torch.zeros_like(t)            # gsr_grow_fold writes the selected rows only
        g = _params(pl, xyz, f_dc, f_rest, opacity, scaling, rotation, learned, dirs, noise)
        gg = _lib.GsrGrowGrads()
        for k in range(7):
            gg.in_[k] = gin[k].data_ptr() if gin[k].numel() else None
            gg.out[k] = gout[k].data_ptr() if gout[k].numel() else None
        for k in _LEARNED:
            setattr(gg, "d_" + k, dl[k].data_ptr() if k in dl else None)
        with torch.cuda.device(dev):
            _lib.check(lib.gsr_grow_fold(C.byref(g), C.byref(gg), torch.cuda.current_stream(dev).cuda_stream),
                       "gsr_grow_fold")
        return (None, None, None, *gout, *(dl.get(k) for k in _LEARNED))


def _noise_for(pl: Plan, mode: int, noise, dev):
    if pl.G == 0 or mode & (_lib.GROW_DIR | _lib.GROW_CONTINUOUS) or mode & _lib.SPLIT_DISTANCE:
        return None
    if noise is None:
        return torch.randn(pl.G, 3, device=dev)        # torch.normal(mean=0, std=stds) of :210-212 draws these
    return noise


def expand(pc, means2D, mode: int, densify_grad_threshold: float, percent_dense_extent: float,
           noise: Optional[torch.Tensor] = None, pl: Optional[Plan] = None):
    """-> (plan, (xyz, means2D, f_dc, f_rest, opacity, scaling, rotation) with P + G rows), differentiable w.r.t. the
    model's raw tensors, ``means2D`` and the learned tensors of the mode.  ``noise``: ``[G, 3]`` standard normal for a
    learned split without ``learn_split_distance`` (default: ``torch.randn`` on the device)."""
    if pl is None:
        pl = plan(pc, mode, densify_grad_threshold, percent_dense_extent)
    noise = _noise_for(pl, mode, noise, pc._xyz.device)
    use = _learned_for(mode)
    learned = [getattr(pc, "_" + k) if use[k] else None for k in _LEARNED]
    dirs = getattr(pc, "dirs", None) if use["dirs_prob"] else None
    out = _GrowExpand.apply(pl, dirs, noise, pc._xyz, means2D, pc._features_dc, pc._features_rest, pc._opacity,
                            pc._scaling, pc._rotation, *learned)
    return pl, out


def percent_dense_extent(pc, which: str, modelcg, cameras_extent) -> float:
    """percent_dense * cameras_extent as the float32 the comparison of :137-138 / :193-194 uses; +inf when no split
    test is made (grow mode without a learned split)."""
    learn_d, learn_s = _split_flags(modelcg)
    if which == GROW and not (learn_d or learn_s):
        return math.inf
    if cameras_extent is None:
        raise ValueError("the learned split needs cameras_extent (gaussian_renderer/__init__.py:189 asserts it)")
    return float(torch.tensor(pc.percent_dense * cameras_extent, dtype=torch.float32))
