"""Generates tests/golden/densify_fork.npz from the reference's own Python (run ONLY where the reference is checked out;
the fixture -- plain arrays -- is committed):

    python tests/golden/make_golden_densify_fork.py

scene/gaussian_model.py densify_and_prune (:751-773) of the fork's models, on CPU: the clone + split branch with the
learned tensors (:509-610) and the grow branch (densify_and_grow :612-677, densify_and_growsplit :679-749), each on a
model with a real torch.optim.Adam state on every group (training_setup :240-266).  The class is loaded as
make_golden_model.py loads it, called under torch.no_grad() (train.py:111/:134) with its prints silenced.

Patches, on top of make_golden_model.py's (factory functions without device="cuda"):
  - torch.normal(mean, std) of :537-539 / :705-708 -> mean + std * z, z stored ("noise": the split's draws in the
    reference's order);
  - torch.randn of the continuous re-init (:650) -> seeded draws, stored ("dir_noise").

Every case is checked for margins first: no grad, largest scale (parent or child), opacity or top-two logit gap lies
within a relative 1e-4 of its threshold, so a float32 implementation with other exp / log roundings makes the same
decisions.
"""
import contextlib
import io
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_model as mgm  # noqa: E402

ATTR = dict(mgm.ATTR, dirs_prob="_dirs_prob", conti_dirs="_conti_dirs", grow_dist="_grow_dist",
            split_distance="_split_distance", split_scale="_split_scale")
FLAG_NAMES = ("grow_dir", "continous_dir", "grow_distance", "learn_split_distance", "learn_split_scale",
              "symmetric_split", "split_notreinit", "prob_notreinit")
RESET = 3000
MARGIN = 1e-4
_randn = torch.randn

# name: (flags, P, num_dirs, iteration, max_grad, min_opacity, max_screen_size)
CASES = {
    "cs_dirs_prob": (dict(grow_dir=True, grow_distance=True), 100, 16, 1500, 0.0002, 0.005, 20),
    "cs_learned": (dict(learn_split_distance=True, learn_split_scale=True), 100, 16, 1500, 0.0002, 0.005, 20),
    "cs_learned_notreinit": (dict(learn_split_distance=True, learn_split_scale=True, split_notreinit=True), 100, 16,
                             1500, 0.0002, 0.005, None),
    "cs_symmetric": (dict(symmetric_split=True, grow_distance=True, learn_split_scale=True), 100, 16, 1500, 0.0002,
                     0.005, 20),
    "grow_dir_distance": (dict(grow_dir=True, grow_distance=True), 100, 24, 3100, 0.0002, 0.005, 20),
    "grow_dir_notreinit": (dict(grow_dir=True, grow_distance=True, prob_notreinit=True), 100, 16, 3100, 0.0002,
                           0.005, None),
    "grow_conti_distance": (dict(continous_dir=True, grow_distance=True), 100, 16, 3100, 0.0002, 0.005, 20),
    "grow_learned_split": (dict(grow_dir=True, learn_split_distance=True, learn_split_scale=True), 100, 16, 3100,
                           0.0002, 0.005, 20),
    "grow_symmetric": (dict(continous_dir=True, symmetric_split=True), 100, 16, 3100, 0.0002, 0.005, 20),
    "grow_nothing_selected": (dict(grow_dir=True, grow_distance=True), 80, 16, 3100, 1.0, 0.005, 20),
    "grow_all_pruned": (dict(grow_dir=True, learn_split_scale=True), 80, 16, 3100, 0.0002, 0.999, 20),
    "grow_dir128": (dict(grow_dir=True, grow_distance=True, learn_split_distance=True), 40, 128, 3100, 0.0002, 0.005,
                    20),
}
EXTENT = 5.0
PERCENT_DENSE = 0.01


def _near(v, t):
    return (v - t).abs() <= MARGIN * max(abs(t), 1e-30)


def _fix_margins(raw, accum, denom, flags, max_grad, min_opacity, g):
    """Nudges the rows whose decisions sit within MARGIN of a threshold; returns the number of rows it touched."""
    touched = 0
    for _ in range(50):
        grad = (accum / denom).double().squeeze(1)
        grad[grad.isnan()] = 0.0
        s = raw["scaling"].double().exp()
        mx = s.max(dim=1).values
        k = 1.6 if not flags.get("learn_split_scale") else \
            (2 * (0.6 * torch.sigmoid(raw["split_scale"].double()) + 0.5)).squeeze(1)
        cmx = mx / k
        op = torch.sigmoid(raw["opacity"].double()).squeeze(1)
        bad = (_near(grad, max_grad) | _near(mx, PERCENT_DENSE * EXTENT) | _near(mx, 0.1 * EXTENT) |
               _near(cmx, 0.1 * EXTENT) | _near(op, min_opacity))
        if "dirs_prob" in raw:
            top = raw["dirs_prob"].double().topk(2, dim=1).values
            bad |= (top[:, 0] - top[:, 1]) < 1e-3
        if not bool(bad.any()):
            return touched
        n = int(bad.sum())
        touched += n
        raw["scaling"][bad] += 0.05 * _randn(n, 3, generator=g)
        raw["opacity"][bad] += 0.05 * _randn(n, 1, generator=g)
        accum[bad] *= 1.0 + 0.05 * torch.rand(n, 1, generator=g)
        if "split_scale" in raw:
            raw["split_scale"][bad] += 0.1 * _randn(n, 1, generator=g)
        if "dirs_prob" in raw:
            raw["dirs_prob"][bad] = _randn(n, raw["dirs_prob"].shape[1], generator=g)
    raise RuntimeError("could not clear the threshold margins")


def build_fork_model(mod, flags, P, num_dirs, max_grad, min_opacity, seed):
    g = torch.Generator().manual_seed(seed)
    cg = types.SimpleNamespace(**{f: bool(flags.get(f, False)) for f in
                                  ("learn_split_distance", "learn_split_scale", "symmetric_split", "split_notreinit",
                                   "prob_notreinit")})
    with mgm._Patched():
        m = mod.GaussianModel(1, grow_dir=bool(flags.get("grow_dir")), num_dirs=num_dirs,
                              continous_dir=bool(flags.get("continous_dir")),
                              grow_distance=bool(flags.get("grow_distance")), modelcg=cg)
    raw = {
        "xyz": _randn(P, 3, generator=g) * 2.0,
        "f_dc": _randn(P, 1, 3, generator=g),
        "f_rest": 0.1 * _randn(P, 3, 3, generator=g),
        "opacity": 2.5 * _randn(P, 1, generator=g) - 1.0,
        "scaling": float(np.log(0.05)) + 1.2 * _randn(P, 3, generator=g),
        "rotation": _randn(P, 4, generator=g),
    }
    if flags.get("grow_dir"):
        raw["dirs_prob"] = _randn(P, num_dirs, generator=g)
    if flags.get("continous_dir"):
        raw["conti_dirs"] = _randn(P, 3, generator=g)
    if flags.get("grow_distance"):
        raw["grow_dist"] = _randn(P, 1, generator=g)
    if flags.get("learn_split_distance"):
        raw["split_distance"] = _randn(P, 3, generator=g)
    if flags.get("learn_split_scale"):
        raw["split_scale"] = 2.0 * _randn(P, 1, generator=g)
    denom = torch.randint(0, 4, (P, 1), generator=g).float()      # zeros -> 0/0 = NaN -> 0 (:752-753)
    accum = torch.rand(P, 1, generator=g) * 0.0006 * denom
    _fix_margins(raw, accum, denom, flags, max_grad, min_opacity, g)
    for k, t in raw.items():
        setattr(m, ATTR[k], torch.nn.Parameter(t.clone().requires_grad_(True)))
    m.active_sh_degree = 1
    m.spatial_lr_scale = 1.0
    args = types.SimpleNamespace(percent_dense=PERCENT_DENSE, position_lr_init=0.00016, position_lr_final=0.0000016,
                                 position_lr_delay_mult=0.01, position_lr_max_steps=30000, feature_lr=0.0025,
                                 opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001, growdirs_lr=0.01,
                                 growdistance_lr=0.01, splitdistance_lr=0.01, splitscale_lr=0.01)
    with mgm._Patched(), contextlib.redirect_stdout(io.StringIO()):
        m.training_setup(args)                                    # :240-266: Adam over every group of the flags
    assert {grp["name"] for grp in m.optimizer.param_groups} == set(raw)
    for k in raw:                                                 # one step creates exp_avg / exp_avg_sq
        p = getattr(m, ATTR[k])
        p.grad = _randn(p.shape, generator=g)
    m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    m.xyz_gradient_accum, m.denom = accum, denom
    m.max_radii2D = torch.floor(torch.rand(P, generator=g) * 40)
    return m, g, list(raw)


def snapshot(m, names, prefix, out):
    for k in names:
        p = getattr(m, ATTR[k])
        out[f"{prefix}/param/{k}"] = p.detach().numpy().copy()
        st = m.optimizer.state[p]
        out[f"{prefix}/exp_avg/{k}"] = st["exp_avg"].numpy().copy()
        out[f"{prefix}/exp_avg_sq/{k}"] = st["exp_avg_sq"].numpy().copy()
    if prefix.endswith("/in"):                                    # after densification: zeros of the new size
        for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
            out[f"{prefix}/{k}"] = getattr(m, k).numpy().copy()
    else:
        assert all(not getattr(m, k).any() and getattr(m, k).shape[0] == m._xyz.shape[0]
                   for k in ("xyz_gradient_accum", "denom", "max_radii2D"))


def main():
    mod = mgm.load_reference_model_module()
    out = {}
    for seed, (case, (flags, P, nd, iteration, max_grad, min_opacity, max_screen_size)) in enumerate(CASES.items()):
        m, g, names = build_fork_model(mod, flags, P, nd, max_grad, min_opacity, seed=100 + seed)
        snapshot(m, names, f"{case}/in", out)
        if flags.get("grow_dir"):
            out[f"{case}/dirs"] = m.dirs.numpy().copy()
        normal_draws, randn_draws = [], []

        def recording_normal(mean=None, std=None, **kw):
            z = _randn(std.shape, generator=g)
            normal_draws.append(z.clone())
            return mean + std * z

        def recording_randn(*size, **kw):
            kw.pop("device", None)
            z = _randn(*size, generator=g, **kw)
            randn_draws.append(z.clone())
            return z

        opt = types.SimpleNamespace(opacity_reset_interval=RESET)
        with mgm._Patched([mock.patch.object(torch, "normal", recording_normal),
                           mock.patch.object(torch, "randn", recording_randn)]), \
                torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            m.densify_and_prune(max_grad, min_opacity, EXTENT, max_screen_size, opt, iteration)
        assert len(normal_draws) <= 1 and len(randn_draws) <= 1, (len(normal_draws), len(randn_draws))
        out[f"{case}/noise"] = (normal_draws[0] if normal_draws else torch.zeros(0, 3)).numpy()
        out[f"{case}/dir_noise"] = (randn_draws[0] if randn_draws else torch.zeros(0, 3)).numpy()
        out[f"{case}/flags"] = np.array([bool(flags.get(f, False)) for f in FLAG_NAMES])
        out[f"{case}/args"] = np.array([max_grad, min_opacity, EXTENT, -1.0 if max_screen_size is None else
                                        max_screen_size, PERCENT_DENSE, iteration, RESET, nd], dtype=np.float64)
        snapshot(m, names, f"{case}/out", out)
        print(f"{case}: P {P} -> {out[f'{case}/out/param/xyz'].shape[0]}, noise {tuple(out[f'{case}/noise'].shape)}, "
              f"dir_noise {tuple(out[f'{case}/dir_noise'].shape)}")
    path = os.path.join(HERE, "densify_fork.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
