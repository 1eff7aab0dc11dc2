"""Generates tests/golden/grow_branch.npz from the reference's own Python (run ONLY where the reference is checked out;
the fixture -- plain arrays -- is committed):

    python tests/golden/make_golden_grow.py

gaussian_renderer/__init__.py render() with its grow / learned-split branch (:91-253), on CPU, with the recording stub
of make_golden_model.py for the absent operator module.  Per case it records the extended tensors the reference hands
its operator (means3D, means2D, shs, opacities, scales, rotations: P + G rows), the stub's radii after the truncation
of :266-269, selected_pts_mask, and -- after backpropagating a seeded linear cotangent over the recorded tensors -- the
gradient of every leaf (the model's raw tensors, its learned grow / split tensors, viewspace_points).

Patches, on top of make_golden_model.py's (factory functions without device="cuda"; ones_like added):
  - torch.normal(mean, std) of :210-212 -> (mean + std * z).detach() with z stored: torch.normal passes no gradient to
    mean or std, and z lets another implementation consume the same draws.
"""
import importlib.util
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_model as mgm  # noqa: E402

P, SH_DEGREE, NUM_DIRS = 128, 3, 128
OPT = dict(densify_from_iter=500, densification_interval=100, densify_until_iter=15000, opacity_reset_interval=3000)
THRESHOLD = 0.0002
LEARNED = ("dirs_prob", "conti_dirs", "grow_dist", "split_distance", "split_scale")
RECORDED = ("means3D", "means2D", "shs", "opacities", "scales", "rotations")

# name: (render kwargs other than opt / modelcg, learn_split_distance, learn_split_scale, cameras_extent)
CASES = {
    "grow_dir": (dict(grow_dir=True, iteration=4000), False, False, 5.0),
    "grow_dir_distance": (dict(grow_dir=True, grow_distance=True, iteration=4000), False, False, 5.0),
    "continous_dir": (dict(continous_dir=True, grow_distance=True, iteration=14999), False, False, 5.0),
    "split_distance": (dict(iteration=100), True, False, 5.0),
    "split_scale": (dict(iteration=100), False, True, 5.0),
    "split_both": (dict(iteration=20000), True, True, 5.0),
    "gate_inner_closed": (dict(grow_dir=True, iteration=3000), True, True, 5.0),
    "grow_split_zero": (dict(grow_dir=True, iteration=4000), True, False, 1.0e6),
    "grow_split_raises": (dict(grow_dir=True, iteration=4000), True, False, 5.0),
}


def cotangent(seed, shapes):
    """The linear cotangent of a case: one standard-normal tensor per recorded tensor, drawn in RECORDED order."""
    gen = torch.Generator().manual_seed(int(seed))
    return {k: torch.randn(tuple(shapes[k]), generator=gen) for k in RECORDED}


def load_renderer(model_mod):
    stub = types.ModuleType("diff_gaussian_rasterization")
    stub.GaussianRasterizationSettings = mgm.RecordedSettings
    stub.GaussianRasterizer = mgm.RecordingRasterizer
    scene_pkg = types.ModuleType("scene")
    scene_pkg.__path__ = []
    sys.modules.update({"diff_gaussian_rasterization": stub, "scene": scene_pkg, "scene.gaussian_model": model_mod})
    spec = importlib.util.spec_from_file_location("ref_gaussian_renderer_grow",
                                                  os.path.join(mgm.REF, "gaussian_renderer", "__init__.py"))
    rmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rmod)
    return rmod


def build(model_mod, seed):
    m, g = mgm.build_model(model_mod, P, SH_DEGREE, seed)
    with torch.no_grad():
        iso = torch.rand(P, generator=g) < 0.25                 # isotropic rows: max over tied scales (distCUDA2 init)
        m._scaling[iso] = m._scaling[iso][:, :1].expand(-1, 3).clone()
    logits = torch.randn(P, NUM_DIRS, generator=g)
    uniform = torch.rand(P, generator=g) < 0.4                  # the 1/num_dirs initialisation: every logit tied
    logits[uniform] = 1.0 / NUM_DIRS
    learned = {"dirs_prob": logits, "conti_dirs": torch.randn(P, 3, generator=g),
               "grow_dist": torch.randn(P, 1, generator=g), "split_distance": torch.randn(P, 3, generator=g),
               "split_scale": torch.randn(P, 1, generator=g)}
    for k, v in learned.items():
        setattr(m, "_" + k, torch.nn.Parameter(v.clone().requires_grad_(True)))
    m.dirs = torch.tensor(model_mod.sphere_points(NUM_DIRS)).to(torch.float32)
    m.percent_dense = 0.01
    denom = torch.randint(0, 4, (P, 1), generator=g).float()
    m.xyz_gradient_accum = torch.rand(P, 1, generator=g) * 0.0006 * denom        # ~ half above THRESHOLD
    m.denom = denom
    return m, g


def run_case(rmod, model_mod, name, seed, case_index):
    kw, learn_d, learn_s, extent = CASES[name]
    m, g = build(model_mod, seed)
    out = {"extent": np.array(extent, dtype=np.float64), "flags": np.array([learn_d, learn_s])}
    model = {"threshold": np.array(THRESHOLD, dtype=np.float64), "percent_dense": np.array(m.percent_dense, dtype=np.float64),
             "dirs": m.dirs.numpy().copy(), "xyz_gradient_accum": m.xyz_gradient_accum.numpy().copy(),
             "denom": m.denom.numpy().copy()}
    for k, a in mgm.ATTR.items():
        model[f"model/{k}"] = getattr(m, a).detach().numpy().copy()
    for k in LEARNED:
        model[f"model/{k}"] = getattr(m, "_" + k).detach().numpy().copy()
    run_case.model = model         # the same model (same seed) in every case
    draws = []

    def recording_normal(mean=None, std=None, **_):
        z = torch.randn(std.shape, generator=g)
        draws.append(z.clone())
        return (mean + std * z).detach()

    cam = types.SimpleNamespace(image_height=24, image_width=32, FoVx=1.1, FoVy=0.8,
                                world_view_transform=torch.eye(4), full_proj_transform=torch.eye(4),
                                camera_center=torch.zeros(3))
    pipe = types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False, debug=False)
    cg = types.SimpleNamespace(learn_split_distance=learn_d, learn_split_scale=learn_s)
    mgm.CALLS.clear()
    patches = [mock.patch.object(torch, "normal", recording_normal),
               mock.patch.object(torch, "ones_like", mgm._drop_device(torch.ones_like))]
    try:
        with mgm._Patched(patches):
            res = rmod.render(cam, m, pipe, torch.zeros(3), densify_grad_threshold=THRESHOLD,
                              opt=types.SimpleNamespace(**OPT), modelcg=cg, cameras_extent=extent, **kw)
    except AssertionError:
        out["raises"] = np.array(True)
        return out
    out["raises"] = np.array(False)
    out["kwargs"] = np.array(sorted(k for k, v in kw.items()))
    for k in ("grow_dir", "continous_dir", "grow_distance"):
        out[f"arg/{k}"] = np.array(bool(kw.get(k, False)))
    out["arg/iteration"] = np.array(kw["iteration"])
    assert len(mgm.CALLS) == 1
    _, rk = mgm.CALLS[0]
    out["noise"] = (draws[0] if draws else torch.zeros(0, 3)).numpy().copy()
    for k in RECORDED:
        out[f"ext/{k}"] = rk[k].detach().numpy().copy()
    out["radii"] = res["radii"].numpy().copy()
    sel = res["selected_pts_mask"]
    out["selected_is_none"] = np.array(sel is None)
    if sel is not None:
        out["selected"] = sel.numpy().copy()
    # the seeded linear cotangent over the recorded tensors (cotangent(): CPU torch.randn, reproducible from the seed)
    out["cotangent_seed"] = np.array(1000 + case_index)
    loss = 0.0
    for k, w in cotangent(1000 + case_index, {k: rk[k].shape for k in RECORDED}).items():
        loss = loss + (w * rk[k]).sum()
    loss.backward()
    none = []
    for k, a in list(mgm.ATTR.items()) + [(k, "_" + k) for k in LEARNED]:
        gr = getattr(m, a).grad
        if gr is None:
            none.append(k)
        else:
            out[f"grad/{k}"] = gr.numpy().copy()
    out["grad/means2D"] = res["viewspace_points"].grad.numpy().copy()
    out["grad_none"] = np.array(sorted(none))
    return out


def main():
    model_mod = mgm.load_reference_model_module()
    rmod = load_renderer(model_mod)
    out = {"opt": np.array([OPT[k] for k in ("densify_from_iter", "densification_interval", "densify_until_iter",
                                             "opacity_reset_interval")]), "cases": np.array(list(CASES))}
    for n, name in enumerate(CASES):
        for k, v in run_case(rmod, model_mod, name, 50, n).items():
            out[f"{name}/{k}"] = v
        out.update(run_case.model)
        G = out[f"{name}/ext/means3D"].shape[0] - P if f"{name}/ext/means3D" in out else -1
        print(f"{name}: G = {G}, raises = {bool(out[f'{name}/raises'])}")
    path = os.path.join(HERE, "grow_branch.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
