"""GaussianModel / trainer host logic without a GPU (mvs_gaussian_splatting_amd/model.py, trainer.py, csrc/model.hip's
exports): ABI surface, the class's names against the reference's (tests/golden/model_lifecycle.npz), the capture()
layout, restore()'s argument handling, the no-CPU-path rule, and the schedule of train.py:72-142 against a table
written out by hand from that file."""
import os
import re
import types

import numpy as np
import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "model_lifecycle.npz")
GROUP_ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
              "scaling": "_scaling", "rotation": "_rotation"}
NEW_SYMBOLS = ("gsr_opacity_sparsity_workspace_bytes", "gsr_opacity_sparsity_fwd", "gsr_opacity_sparsity_bwd",
               "gsr_reset_opacity")


def fixture_opt(fx):
    return types.SimpleNamespace(**{str(k): float(v) for k, v in zip(fx["reset/opt_names"], fx["reset/opt_values"])})


def cpu_plain_model(fx, optimizer_cls=torch.optim.Adam):
    """The reset case's model before the reset, on the CPU, with its Adam state."""
    from mvs_gaussian_splatting_amd.model import GaussianModel
    m = GaussianModel(0)
    for k, a in GROUP_ATTR.items():
        setattr(m, a, nn.Parameter(torch.from_numpy(fx[f"reset/before/param/{k}"]).clone().requires_grad_(True)))
    m.spatial_lr_scale = float(fx["reset/spatial_lr_scale"])
    P = m._xyz.shape[0]
    m.max_radii2D = torch.zeros(P)
    m.training_setup(fixture_opt(fx), optimizer_cls)
    for k, a in GROUP_ATTR.items():
        m.optimizer.state[getattr(m, a)] = {"step": torch.tensor(float(fx[f"reset/before/step/{k}"])),
                                            "exp_avg": torch.from_numpy(fx[f"reset/before/exp_avg/{k}"]).clone(),
                                            "exp_avg_sq": torch.from_numpy(fx[f"reset/before/exp_avg_sq/{k}"]).clone()}
    return m


def test_new_symbols_are_exported_and_abi_numbers_agree():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS and re.search(rf"\b{name}\s*\(", header), name
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version()
    assert lib.gsr_opacity_sparsity_workspace_bytes() >= 2048 * 8
    # arguments are refused before any launch
    assert lib.gsr_opacity_sparsity_fwd(None, 4, 1.0, 0.005, None, None, None) == -1
    assert lib.gsr_opacity_sparsity_bwd(None, 4, 0.005, None, None, None, None) == -1
    assert lib.gsr_reset_opacity(None, 4, 0.01, None, None, None) == -1
    assert lib.gsr_reset_opacity(None, -1, 0.01, None, None, None) == -1
    assert lib.gsr_reset_opacity(None, 0, 1.5, None, None, None) == -1 and b"cap" in lib.gsr_last_error()
    assert lib.gsr_reset_opacity(None, 0, 0.01, None, None, None) == 0


def test_class_names_match_the_reference():
    from mvs_gaussian_splatting_amd import GaussianModel
    fx = np.load(FIXTURE)
    for name in fx["api/methods"]:
        assert callable(getattr(GaussianModel, str(name))), name
    for name in fx["api/properties"]:
        assert isinstance(getattr(GaussianModel, str(name)), property), name
    cases = {"plain": dict(), "grow_dir": dict(grow_dir=True, num_dirs=128), "continous_dir": dict(continous_dir=True),
             "dist_splits": dict(grow_distance=True, modelcg=types.SimpleNamespace(learn_split_distance=True,
                                                                                   learn_split_scale=True))}
    for tag, kw in cases.items():
        m = GaussianModel(int(fx[f"pcd/{tag}/sh_degree"]), **kw)
        have = set(vars(m))
        missing = {str(n) for n in fx[f"pcd/{tag}/fresh_attrs"]} - have
        assert not missing, (tag, missing)
        assert m.active_sh_degree == 0 and m.max_sh_degree == int(fx[f"pcd/{tag}/sh_degree"])
        assert m.optimizer is None and m._xyz.numel() == 0
    # a tensor exists exactly when its flag is set (densify._fork_inputs relies on it)
    plain = GaussianModel(3)
    for a in ("_dirs_prob", "_conti_dirs", "_grow_dist", "_split_distance", "_split_scale", "dirs"):
        assert not hasattr(plain, a)
    assert plain.scaling_activation is torch.exp and plain.opacity_activation is torch.sigmoid
    assert plain.rotation_activation is torch.nn.functional.normalize


def test_sphere_points_match_the_reference():
    from mvs_gaussian_splatting_amd.model import GaussianModel, sphere_points
    fx = np.load(FIXTURE)
    assert np.array_equal(sphere_points(128), fx["sphere_points_128"])
    m = GaussianModel(3, grow_dir=True, num_dirs=128)
    assert m.dirs.dtype == torch.float32 and np.array_equal(m.dirs.numpy(), fx["pcd/grow_dir/dirs"])


def test_oneup_sh_degree_saturates():
    from mvs_gaussian_splatting_amd import GaussianModel
    m = GaussianModel(2)
    seen = []
    for _ in range(4):
        m.oneupSHdegree()
        seen.append(m.active_sh_degree)
    assert seen == [1, 2, 2, 2]


def test_getters_on_cpu_tensors_match_the_synthetic_model():
    from mvs_gaussian_splatting_amd import GaussianModel
    from mvs_gaussian_splatting_amd.synthetic import SyntheticGaussianModel
    s = SyntheticGaussianModel(50, 2, seed=3)
    m = GaussianModel(2)
    for a in GROUP_ATTR.values():
        setattr(m, a, getattr(s, a))
    for name in ("get_xyz", "get_scaling", "get_rotation", "get_opacity", "get_features"):
        assert torch.equal(getattr(m, name), getattr(s, name)), name
    assert torch.equal(m.get_covariance(1.3), s.get_covariance(1.3))


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_capture_layout_of_a_plain_model(optimizer):
    from mvs_gaussian_splatting_amd import optim
    fx = np.load(FIXTURE)
    m = cpu_plain_model(fx, torch.optim.Adam if optimizer == "torch" else optim.Adam)
    cap = m.capture()
    assert len(cap) == int(fx["capture/length"]) == 12
    assert [type(v).__name__ for v in cap] == [str(s) for s in fx["capture/types"]]
    want_shapes = [str(s) for s in fx["capture/shapes"]]
    for i, v in enumerate(cap):
        if torch.is_tensor(v):
            if i not in (8, 9):                       # xyz_gradient_accum / denom: zeros here, [P,1] in both
                assert ",".join(map(str, v.shape)) == want_shapes[i], i
            assert str(v.dtype) == str(fx["capture/dtypes"][i]), i
    assert cap[0] == m.active_sh_degree and cap[1] is m._xyz and cap[6] is m._opacity and cap[11] == m.spatial_lr_scale
    sd = cap[10]
    assert sorted(sd.keys()) == [str(s) for s in fx["capture/state_dict_keys"]]
    assert sorted(sd["state"].keys()) == [int(i) for i in fx["capture/state_ids"]]
    assert sorted(sd["state"][0].keys()) == [str(s) for s in fx["capture/state_keys"]]
    assert [g["name"] for g in sd["param_groups"]] == [str(s) for s in fx["capture/group_names"]]
    assert set(str(s) for s in fx["capture/group_keys"]) <= set(sd["param_groups"][0].keys())


def test_restore_takes_12_or_13_elements():
    from mvs_gaussian_splatting_amd import GaussianModel, optim
    fx = np.load(FIXTURE)
    opt = fixture_opt(fx)
    src = cpu_plain_model(fx)
    src.active_sh_degree = 0
    cap = src.capture()
    dst = GaussianModel(0)
    dst.restore(cap, opt, torch.optim.Adam)
    assert isinstance(dst.optimizer, torch.optim.Adam) and dst._xyz is src._xyz
    assert dst.xyz_gradient_accum is src.xyz_gradient_accum and dst.spatial_lr_scale == src.spatial_lr_scale
    st = dst.optimizer.state[dst._opacity]
    assert float(st["step"]) == 2.0 and torch.equal(st["exp_avg"], src.optimizer.state[src._opacity]["exp_avg"])
    # the state moves between the two optimizer classes; the default is this package's Adam
    dst2 = GaussianModel(0)
    dst2.restore(cap, opt)
    assert isinstance(dst2.optimizer, optim.Adam)
    assert torch.equal(dst2.optimizer.state[dst2._xyz]["exp_avg_sq"], src.optimizer.state[src._xyz]["exp_avg_sq"])
    with pytest.raises(ValueError, match="12- or 13-element"):
        GaussianModel(0).restore(cap[:11], opt)
    # a fork model: 13th element, the dict of its learned tensors
    cg = types.SimpleNamespace(learn_split_distance=True, learn_split_scale=False)
    fork = GaussianModel(0, grow_dir=True, num_dirs=8, modelcg=cg)
    P = src._xyz.shape[0]
    for a in GROUP_ATTR.values():
        setattr(fork, a, nn.Parameter(getattr(src, a).detach().clone().requires_grad_(True)))
    fork._dirs_prob = nn.Parameter(torch.full((P, 8), 0.125).requires_grad_(True))
    fork._split_distance = nn.Parameter(torch.zeros(P, 3).requires_grad_(True))
    fork.max_radii2D = torch.zeros(P)
    fork.training_setup(opt, torch.optim.Adam)
    cap13 = fork.capture()
    assert len(cap13) == 13 and sorted(cap13[12]) == ["_dirs_prob", "_split_distance"]
    assert [g["name"] for g in cap13[10]["param_groups"]][6:] == ["dirs_prob", "split_distance"]
    again = GaussianModel(0, grow_dir=True, num_dirs=8, modelcg=cg)
    again.restore(cap13, opt, torch.optim.Adam)
    assert again._dirs_prob is fork._dirs_prob and len(again.optimizer.param_groups) == 8
    with pytest.raises(ValueError, match="learned tensors"):
        GaussianModel(0).restore(cap13, opt)                         # a plain model cannot take a fork checkpoint
    with pytest.raises(ValueError, match="learned tensors"):
        GaussianModel(0, grow_dir=True, num_dirs=8, modelcg=cg).restore(cap, opt)


def test_no_cpu_path():
    from mvs_gaussian_splatting_amd import GaussianModel, _lib, opacity_sparsity_loss
    fx = np.load(FIXTURE)
    m = cpu_plain_model(fx)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        m.reset_opacity()
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        opacity_sparsity_loss(m._opacity, 0.05)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        opacity_sparsity_loss(m._opacity, 0.0)                       # even the free path refuses CPU tensors
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        GaussianModel(3).create_from_pcd(torch.from_numpy(fx["pcd/points"]), torch.from_numpy(fx["pcd/colors"]), 1.0)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.GsrError, match="no CPU path"):
            GaussianModel(3).create_from_pcd(fx["pcd/points"], fx["pcd/colors"], 1.0)
        with pytest.raises(_lib.GsrError, match="no CPU path"):
            GaussianModel(3).load_ply(os.path.join(ROOT, "does-not-matter.ply"))


def test_optimization_params_defaults():
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams
    o = OptimizationParams()
    # arguments/__init__.py:84-107
    want = dict(iterations=30_000, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
                position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001,
                percent_dense=0.01, growdirs_lr=0.005, growdistance_lr=0.001, lambda_dssim=0.2,
                densification_interval=100, opacity_reset_interval=3000, densify_from_iter=500,
                densify_until_iter=15_000, densify_grad_threshold=0.0002, min_opacity=0.005, random_background=False,
                opacitysparse=0.0, splitdistance_lr=0.005, splitscale_lr=0.005)
    for k, v in want.items():
        assert getattr(o, k) == v, k
    assert OptimizationParams(opacitysparse=0.1).opacitysparse == 0.1 and OptimizationParams.opacitysparse == 0.0
    with pytest.raises(TypeError):
        OptimizationParams(no_such_field=1)


# train.py:72-142 by hand, default OptimizationParams (iterations 30000, densify 500 < it < 15000 every 100, reset every
# 3000): iteration -> (degree-up :75, statistics :127, densify :132, size_threshold :133, reset :136 black background,
# reset :136 white background, optimizer step :140)
SCHEDULE = {
    499:   (False, True,  False, None, False, False, True),
    500:   (False, True,  False, None, False, True,  True),    # 500 > 500 is false: no densify; white: first reset
    501:   (False, True,  False, None, False, False, True),
    600:   (False, True,  True,  None, False, False, True),
    1000:  (True,  True,  True,  None, False, False, True),
    3000:  (True,  True,  True,  None, True,  True,  True),    # 3000 > 3000 is false: size_threshold still None
    3001:  (False, True,  False, 20,   False, False, True),
    14999: (False, True,  False, 20,   False, False, True),
    15000: (True,  False, False, 20,   False, False, True),    # 15000 < 15000 is false: the window is closed
    30000: (True,  False, False, 20,   False, False, False),   # the last iteration does not step
}


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, name):
        def fn(*a, **kw):
            self.calls.append((name, a, kw))
        return fn


class _StubModel:
    def __init__(self, rec):
        self.rec = rec
        self._opacity = torch.zeros(4, 1, requires_grad=True)
        self.optimizer = types.SimpleNamespace(step=rec("step"), zero_grad=rec("zero_grad"))
        self.update_learning_rate = rec("update_learning_rate")
        self.oneupSHdegree = rec("oneupSHdegree")
        self.reset_opacity = rec("reset_opacity")


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("iteration", sorted(SCHEDULE))
def test_training_iteration_follows_the_reference_schedule(monkeypatch, iteration, white):
    from mvs_gaussian_splatting_amd import trainer
    rec = _Recorder()
    model = _StubModel(rec)
    leaf = torch.zeros(3, 4, 4, requires_grad=True)

    def render(cam, pc, pipe, bg, **kw):
        rec.calls.append(("render", (cam, pc, pipe, bg), kw))
        return {"render": leaf * 1.0, "viewspace_points": "vsp", "radii": "radii", "visibility_filter": None,
                "selected_pts_mask": None}

    def loss(img, gt, lam):
        rec.calls.append(("l1_dssim_loss", (gt, lam), {}))
        return img.sum()

    def sparsity(raw, w):
        rec.calls.append(("opacity_sparsity_loss", (raw, w), {}))
        return raw.sum() * 0.0

    monkeypatch.setattr(trainer, "render", render)
    monkeypatch.setattr(trainer, "l1_dssim_loss", loss)
    monkeypatch.setattr(trainer, "opacity_sparsity_loss", sparsity)
    monkeypatch.setattr(trainer, "add_densification_stats", rec("add_densification_stats"))
    monkeypatch.setattr(trainer, "densify_and_prune", rec("densify_and_prune"))
    opt = trainer.OptimizationParams(opacitysparse=0.03)
    dataset = types.SimpleNamespace(white_background=white, grow_dir=True, continous_dir=False, grow_distance=True)
    cam = types.SimpleNamespace(original_image=torch.ones(3, 4, 4))
    bg = torch.zeros(3)
    out = trainer.training_iteration(model, cam, opt, "pipe", bg, iteration, dataset=dataset, cameras_extent=4.5)
    assert isinstance(out, torch.Tensor) and out.dim() == 0 and not out.requires_grad
    names = [c[0] for c in rec.calls]
    sh_up, stats, densify, size_thr, reset_black, reset_white, step = SCHEDULE[iteration]
    reset = reset_white if white else reset_black
    want = ["update_learning_rate"] + (["oneupSHdegree"] if sh_up else []) + ["render", "l1_dssim_loss",
                                                                               "opacity_sparsity_loss"]
    want += (["add_densification_stats"] if stats else []) + (["densify_and_prune"] if densify else [])
    want += (["reset_opacity"] if reset else []) + (["step", "zero_grad"] if step else [])
    assert names == want                                             # the reference's order, nothing else
    by = {c[0]: c for c in rec.calls}
    assert by["update_learning_rate"][1] == (iteration,)
    _, (rcam, rpc, rpipe, rbg), kw = by["render"]
    assert rcam is cam and rpc is model and rpipe == "pipe" and rbg is bg
    assert kw == dict(grow_dir=True, densify_grad_threshold=opt.densify_grad_threshold, iteration=iteration, opt=opt,
                      continous_dir=False, grow_distance=True, modelcg=dataset, cameras_extent=4.5)   # train.py:91
    assert by["l1_dssim_loss"][1][1] == opt.lambda_dssim
    assert by["opacity_sparsity_loss"][1] == (model._opacity, 0.03)
    if stats:
        assert by["add_densification_stats"][1] == (model, "vsp", "radii")
    if densify:
        _, a, kw = by["densify_and_prune"]
        assert a == (model, opt.densify_grad_threshold, opt.min_opacity, 4.5, size_thr)
        assert kw == dict(opt=opt, iteration=iteration)
    if step:
        assert by["zero_grad"][2] == dict(set_to_none=True)
    assert leaf.grad is not None                                     # backward ran


def test_schedule_options(monkeypatch):
    from mvs_gaussian_splatting_amd import trainer
    opt = trainer.OptimizationParams()
    for it, row in SCHEDULE.items():
        for white in (False, True):
            s = trainer.schedule(opt, it, white)
            assert (s["sh_up"], s["stats"], s["densify"], s["reset"], s["step"]) == \
                (row[0], row[1], row[2], row[5] if white else row[4], row[6]), (it, white)
            assert s["size_threshold"] == row[3]
    # opacitysparse = 0 (the default) never calls the term; random_background draws a fresh one; first_reset overrides
    rec = _Recorder()
    model = _StubModel(rec)
    leaf = torch.zeros(3, 2, 2, requires_grad=True)
    seen = {}

    def render(cam, pc, pipe, bg, **kw):
        seen["bg"] = bg
        return {"render": leaf * 1.0, "viewspace_points": None, "radii": None}

    monkeypatch.setattr(trainer, "render", render)
    monkeypatch.setattr(trainer, "l1_dssim_loss", lambda img, gt, lam: img.sum())
    monkeypatch.setattr(trainer, "opacity_sparsity_loss", rec("opacity_sparsity_loss"))
    monkeypatch.setattr(trainer, "add_densification_stats", rec("add_densification_stats"))
    monkeypatch.setattr(trainer, "densify_and_prune", rec("densify_and_prune"))
    opt = trainer.OptimizationParams(random_background=True)
    bg = torch.zeros(3)
    cam = types.SimpleNamespace(original_image=torch.ones(3, 2, 2))
    trainer.training_iteration(model, cam, opt, None, bg, 500, cameras_extent=1.0, first_reset=True)
    names = [c[0] for c in rec.calls]
    assert "opacity_sparsity_loss" not in names and "reset_opacity" in names
    assert seen["bg"] is not bg and seen["bg"].shape == (3,)
