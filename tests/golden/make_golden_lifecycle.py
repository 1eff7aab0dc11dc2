"""Generates tests/golden/model_lifecycle.npz from the reference's own Python (run ONLY where /root/reference exists;
the fixture -- plain arrays and name lists -- is committed):

    python tests/golden/make_golden_lifecycle.py

It pins the lifecycle of the reference's GaussianModel (scene/gaussian_model.py) that mvs_gaussian_splatting_amd/model.py
restates, and the opacity sparsity term of train.py:102-106:
  * create_from_pcd :200-238 for four flag sets (plain, grow_dir, continous_dir, grow_distance + both learned splits);
  * reset_opacity :312-315 with replace_tensor_to_optimizer :386-399 on a model with a real Adam state, and the
    optimizer step that follows it (train.py:136-141: the fresh Parameter has no .grad, so the opacity group is skipped);
  * the sparsity term, restated here on the reference's get_opacity and utils/loss_utils.py l1_loss;
  * the layout of capture() :118-131 of a plain model; sphere_points(128) (utils/general_utils.py:135-148); the
    attribute names of a fresh model.
The reference module is loaded as make_golden_model.py loads it (stub plyfile / simple_knn, torch factory functions
without their device="cuda").  Additionally Tensor.cuda returns the tensor itself, and distCUDA2 returns an array the
fixture stores: the exact mean squared distance to the three nearest neighbours from scipy.spatial.cKDTree, with a few
entries forced below 1e-7 so that the clamp of :210 is exercised.
"""
import math
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_model import ATTR, OUT, _Patched, load_reference_model_module  # noqa: E402

FORK = {"dirs_prob": "_dirs_prob", "conti_dirs": "_conti_dirs", "grow_dist": "_grow_dist",
        "split_distance": "_split_distance", "split_scale": "_split_scale"}
OPT = dict(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
           position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001,
           growdirs_lr=0.005, growdistance_lr=0.001, splitdistance_lr=0.005, splitscale_lr=0.005)
# the methods model.py restates, each checked below to exist on the reference's class
METHODS = ("capture", "restore", "oneupSHdegree", "create_from_pcd", "training_setup", "update_learning_rate",
           "save_ply", "load_ply", "reset_opacity", "get_covariance")
PROPERTIES = ("get_scaling", "get_grow_dist", "get_split_distance", "get_split_scale", "get_rotation", "get_xyz",
              "get_features", "get_opacity", "get_dirs_prob", "get_conti_dirs")


def cg(**kw):
    base = dict(learn_split_distance=False, learn_split_scale=False, symmetric_split=False, split_notreinit=False,
                prob_notreinit=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def cuda_is_identity():
    return mock.patch.object(torch.Tensor, "cuda", lambda self, *a, **k: self)


def make_pcd_cases(mod, out):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(5)
    N = 1500
    pts = (rng.standard_normal((N, 3)) * np.array([2.0, 1.0, 1.5])).astype(np.float32)
    pts[7] = pts[6]                                   # a duplicate pair: its three neighbours are not all at distance 0
    cols = rng.random((N, 3)).astype(np.float32)
    d, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=4)
    dist2 = (d[:, 1:] ** 2).mean(axis=1).astype(np.float32)
    out["pcd/dist2_exact"] = dist2.copy()             # what distCUDA2 must give on these points
    dist2[[3, 40, 900]] = np.array([0.0, 3e-8, 9.9e-8], dtype=np.float32)
    assert (dist2 < 1e-7).sum() == 3
    out["pcd/points"], out["pcd/colors"], out["pcd/dist2"] = pts, cols, dist2
    out["pcd/spatial_lr_scale"] = np.array(3.25)
    mod.distCUDA2 = lambda x: torch.from_numpy(dist2.copy())
    cases = {
        "plain": dict(sh=3, kw={}, cg=cg()),
        "grow_dir": dict(sh=3, kw=dict(grow_dir=True, num_dirs=128), cg=cg()),
        "continous_dir": dict(sh=2, kw=dict(continous_dir=True), cg=cg()),
        "dist_splits": dict(sh=1, kw=dict(grow_distance=True), cg=cg(learn_split_distance=True, learn_split_scale=True)),
    }
    g = torch.Generator().manual_seed(17)
    for tag, c in cases.items():
        draws = []
        real_randn = torch.randn

        def recording_randn(*size, **kw):
            kw.pop("device", None)
            z = real_randn(*size, generator=g, **kw)
            draws.append(z.clone())
            return z

        with _Patched([cuda_is_identity()]), mock.patch.object(torch, "randn", recording_randn):
            m = mod.GaussianModel(c["sh"], modelcg=c["cg"], **c["kw"])
            fresh = sorted(vars(m).keys())
            m.create_from_pcd(types.SimpleNamespace(points=pts, colors=cols), 3.25)
        out[f"pcd/{tag}/sh_degree"] = np.array(c["sh"])
        out[f"pcd/{tag}/fresh_attrs"] = np.array(fresh)
        out[f"pcd/{tag}/active_sh_degree"] = np.array(m.active_sh_degree)
        for k, a in {**ATTR, **FORK}.items():
            if hasattr(m, a) and getattr(m, a).numel() > 0:
                out[f"pcd/{tag}/{k}"] = getattr(m, a).detach().numpy().copy()
        out[f"pcd/{tag}/max_radii2D"] = m.max_radii2D.numpy().copy()
        if c["kw"].get("grow_dir"):
            out[f"pcd/{tag}/dirs"] = m.dirs.numpy().copy()
        if c["kw"].get("continous_dir"):
            assert len(draws) == 1
            out[f"pcd/{tag}/dir_noise"] = draws[0].numpy()
        else:
            assert not draws
    assert out["pcd/plain/opacity"].shape == (N, 1) and out["pcd/grow_dir/dirs_prob"].shape == (N, 128)


def adam_snapshot(m, prefix, out):
    for grp in m.optimizer.param_groups:
        k, p = grp["name"], grp["params"][0]
        st = m.optimizer.state[p]
        out[f"{prefix}/param/{k}"] = p.detach().numpy().copy()
        out[f"{prefix}/exp_avg/{k}"] = st["exp_avg"].numpy().copy()
        out[f"{prefix}/exp_avg_sq/{k}"] = st["exp_avg_sq"].numpy().copy()
        out[f"{prefix}/step/{k}"] = np.array(float(st["step"]))


def make_reset_case(mod, out):
    g = torch.Generator().manual_seed(23)
    P, sh = 1000, 0              # degree 0: an empty f_rest group rides along
    m = mod.GaussianModel(sh, modelcg=cg())
    raw = {"xyz": torch.randn(P, 3, generator=g), "f_dc": torch.randn(P, 1, 3, generator=g),
           "f_rest": 0.1 * torch.randn(P, (sh + 1) ** 2 - 1, 3, generator=g),
           "opacity": math.log(0.01 / 0.99) + 2.0 * torch.randn(P, 1, generator=g),      # straddles sigmoid = 0.01
           "scaling": math.log(0.05) + torch.randn(P, 3, generator=g), "rotation": torch.randn(P, 4, generator=g)}
    for k, a in ATTR.items():
        setattr(m, a, torch.nn.Parameter(raw[k].clone().requires_grad_(True)))
    m.active_sh_degree, m.spatial_lr_scale = 0, 1.5
    args = types.SimpleNamespace(**OPT)
    with _Patched():
        m.training_setup(args)
    for _ in range(2):
        for a in ATTR.values():
            p = getattr(m, a)
            p.grad = torch.randn(p.shape, generator=g)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
    m.max_radii2D = torch.floor(torch.rand(P, generator=g) * 30)
    m.xyz_gradient_accum = torch.rand(P, 1, generator=g)
    m.denom = torch.randint(0, 5, (P, 1), generator=g).float()
    o = torch.sigmoid(m._opacity.detach())
    assert int((o > 0.011).sum()) > 300 and int((o < 0.009).sum()) > 300
    out["reset/spatial_lr_scale"] = np.array(1.5)
    out["reset/opt_names"] = np.array(sorted(OPT))
    out["reset/opt_values"] = np.array([OPT[k] for k in sorted(OPT)], dtype=np.float64)
    adam_snapshot(m, "reset/before", out)

    # ---- capture() of this plain model :118-131: layout only -------------------------------------------------------
    cap = m.capture()
    out["capture/length"] = np.array(len(cap))
    out["capture/types"] = np.array([type(v).__name__ for v in cap])
    out["capture/shapes"] = np.array([",".join(map(str, v.shape)) if torch.is_tensor(v) else "" for v in cap])
    out["capture/dtypes"] = np.array([str(v.dtype) if torch.is_tensor(v) else "" for v in cap])
    sd = cap[10]
    out["capture/state_dict_keys"] = np.array(sorted(sd.keys()))
    out["capture/state_keys"] = np.array(sorted(sd["state"][0].keys()))
    out["capture/state_ids"] = np.array(sorted(sd["state"].keys()))
    out["capture/group_names"] = np.array([grp["name"] for grp in sd["param_groups"]])
    out["capture/group_keys"] = np.array(sorted(sd["param_groups"][0].keys()))

    with _Patched():
        old = m._opacity
        m.reset_opacity()
    assert m._opacity is not old and m._opacity.grad is None
    adam_snapshot(m, "reset/after", out)
    for key in [k for k in out if k.startswith("reset/after/") and not k.endswith("/opacity")]:
        assert np.array_equal(out[key], out[key.replace("/after/", "/before/")]), key
        del out[key]                                  # the other groups are untouched: only the opacity group is stored
    moved = (out["reset/after/param/opacity"] != out["reset/before/param/opacity"])
    below = torch.sigmoid(torch.from_numpy(out["reset/before/param/opacity"])) < 0.01
    # rows below the cap make the sigmoid -> log(x / (1 - x)) round trip; in float32 it returns most of them unchanged
    print("reset_opacity: uncapped rows", int(below.sum()), "of which moved by the round trip", int(moved[below.numpy()].sum()))

    # ---- train.py:136-141: .grad everywhere, reset, step ------------------------------------------------------------
    for grp in m.optimizer.param_groups:
        p = grp["params"][0]
        p.grad = torch.randn(p.shape, generator=g)
        out[f"reset/grad/{grp['name']}"] = p.grad.numpy().copy()
    with _Patched():
        m.reset_opacity()
    assert m._opacity.grad is None
    m.optimizer.step()
    adam_snapshot(m, "reset/after_step", out)
    assert out["reset/after_step/step/opacity"] == 2.0 and out["reset/after_step/step/xyz"] == 3.0
    assert not out["reset/after_step/exp_avg/opacity"].any()


def make_sparsity_cases(mod, out):
    sys.path.insert(0, "/root/reference")
    from utils.loss_utils import l1_loss
    from utils.general_utils import sphere_points
    out["sphere_points_128"] = sphere_points(128)
    g = torch.Generator().manual_seed(31)
    P, w = 4000, 0.05
    cut = math.log(0.005 / 0.995)
    hi = cut + 0.3 + (3.0 - cut - 0.3) * torch.rand(P, 1, generator=g)
    lo = cut - 0.3 - 4.0 * torch.rand(P, 1, generator=g)
    some = torch.where(torch.rand(P, 1, generator=g) < 0.2, lo, hi)
    one = hi.clone()
    one[1234] = lo[1234]
    cases = {"some": some, "one": one, "none": hi.clone()}
    out["sparsity/weight"] = np.array(w)
    opt = types.SimpleNamespace(opacitysparse=w)
    for tag, raw in cases.items():
        raw = raw.float()
        o64 = torch.sigmoid(raw.double())
        assert float((o64 - 0.005).abs().min()) >= 1e-5, "a row too close to the threshold"
        res = {}
        for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            gaussians = mod.GaussianModel(0, modelcg=cg())
            gaussians._opacity = torch.nn.Parameter(raw.to(dtype).clone().requires_grad_(True))
            loss = torch.zeros((), dtype=dtype)
            # train.py:102-106
            prune_mask = (gaussians.get_opacity < 0.005).squeeze()
            n = int(torch.sum(prune_mask))
            if opt.opacitysparse > 0 and torch.sum(prune_mask) > 0:
                opacity_Ll1 = opt.opacitysparse * l1_loss(gaussians.get_opacity[prune_mask], 1)
                loss = loss + opacity_Ll1
                loss.backward()
                grad = gaussians._opacity.grad
            else:
                grad = torch.zeros_like(raw, dtype=dtype)
            res[name] = (loss.detach(), grad, n)
        assert res["f32"][2] == res["f64"][2]
        out[f"sparsity/{tag}/raw"] = raw.numpy().copy()
        out[f"sparsity/{tag}/n"] = np.array(res["f64"][2])
        out[f"sparsity/{tag}/value_f32"] = res["f32"][0].numpy().copy()
        out[f"sparsity/{tag}/value_f64"] = res["f64"][0].numpy().copy()
        out[f"sparsity/{tag}/grad_f64"] = res["f64"][1].numpy().copy()
    assert 600 < out["sparsity/some/n"] < 1000 and out["sparsity/one/n"] == 1 and out["sparsity/none/n"] == 0


def make_api_lists(mod, out):
    for name in METHODS:
        assert callable(getattr(mod.GaussianModel, name)), name
    for name in PROPERTIES:
        assert isinstance(getattr(mod.GaussianModel, name), property), name
    out["api/methods"] = np.array(METHODS)
    out["api/properties"] = np.array(PROPERTIES)


if __name__ == "__main__":
    mod = load_reference_model_module()
    out = {}
    make_pcd_cases(mod, out)
    make_reset_case(mod, out)
    make_sparsity_cases(mod, out)
    make_api_lists(mod, out)
    for k, v in out.items():
        assert v.dtype != object, k
    path = os.path.join(OUT, "model_lifecycle.npz")
    np.savez_compressed(path, **out)
    print("wrote model_lifecycle.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")
