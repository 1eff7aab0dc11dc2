"""Per-image exposure compensation, the part that runs without a GPU: the ABI surface (v23), the new
``OptimizationParams`` defaults, the exposure learning-rate schedule, ``exposure.json``, the model's exposure tensors and
checkpoint forms, and the refusal of CPU tensors.  The kernels are checked in tests/test_gpu_exposure.py."""
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from exposure_restate import A_TRUE, backward64, forward64
from test_model_host import FIXTURE, ROOT, cpu_plain_model, fixture_opt

NEW_SYMBOLS = ("gsr_exposure_workspace_bytes", "gsr_exposure_apply_fwd", "gsr_exposure_apply_bwd")


def test_entry_points_are_exported_and_the_three_abi_numbers_agree():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS and re.search(rf"\b{name}\s*\(", header), name
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 23
    # 12 doubles per block, at least one block, and a cap that keeps the finishing step small
    assert lib.gsr_exposure_workspace_bytes(5, 7) >= 12 * 8
    assert lib.gsr_exposure_workspace_bytes(270, 480) == lib.gsr_exposure_workspace_bytes(1080, 1920) <= 1 << 20
    # arguments are refused before any launch
    assert lib.gsr_exposure_apply_fwd(None, None, 4, 4, None, None) == -1
    assert lib.gsr_exposure_apply_bwd(None, None, None, 4, 4, None, None, None, None) == -1
    assert lib.gsr_exposure_apply_fwd(None, None, 0, 4, None, None) == -1


def test_the_makefile_builds_the_unit_without_contraction():
    mk = open(os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS = .*\bexposure\.o\b", mk, re.M)
    assert re.search(r"^CONTRACT_OFF_OBJS :?\+?= *exposure\.o\b", mk, re.M)
    flags = re.search(r"^\$\(CONTRACT_OFF_OBJS\): (\w+) \+= -ffp-contract=off$", mk, re.M)
    assert flags and re.search(r"^%\.o: %\.hip.*\n\t.*\$\(" + flags.group(1) + r"\)", mk, re.M)


def test_optimization_params_carry_upstreams_exposure_defaults():
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams
    o = OptimizationParams()
    assert (o.exposure_lr_init, o.exposure_lr_final, o.exposure_lr_delay_steps, o.exposure_lr_delay_mult) == \
        (0.01, 0.001, 0, 0.0)
    assert OptimizationParams(exposure_lr_init=0.0).exposure_lr_init == 0.0


def _model_with_exposures(names, opt):
    from mvs_gaussian_splatting_amd import optim
    m = cpu_plain_model(np.load(FIXTURE), optim.Adam)
    m.setup_exposures(names, device="cpu")
    m.training_setup(opt, optim.Adam)
    return m


def test_exposure_schedule_follows_expon_lr_func():
    from mvs_gaussian_splatting_amd import optim
    opt = fixture_opt(np.load(FIXTURE))
    opt.iterations = 3000
    for k, v in dict(exposure_lr_init=0.01, exposure_lr_final=0.001, exposure_lr_delay_steps=0,
                     exposure_lr_delay_mult=0.0).items():
        setattr(opt, k, v)
    m = _model_with_exposures(["a", "b"], opt)
    assert isinstance(m.exposure_optimizer, optim.Adam) and not isinstance(m.exposure_optimizer, optim.SparseGaussianAdam)
    group, = m.exposure_optimizer.param_groups
    assert group["params"][0] is m._exposure and group["lr"] == 0.0 and group["eps"] == 1e-8
    assert tuple(group["betas"]) == (0.9, 0.999)
    want = {0: 0.01, 3000: 0.001, 1500: math.sqrt(0.01 * 0.001)}
    for it, lr in want.items():
        m.update_learning_rate(it)
        assert abs(group["lr"] - lr) <= 1e-12 * lr, (it, group["lr"], lr)
    # a namespace without the four fields gets upstream's defaults
    bare = fixture_opt(np.load(FIXTURE))
    bare.iterations = 3000
    assert not hasattr(bare, "exposure_lr_init")
    m2 = _model_with_exposures(["a"], bare)
    m2.update_learning_rate(1500)
    assert abs(m2.exposure_optimizer.param_groups[0]["lr"] - want[1500]) <= 1e-12 * want[1500]
    # all four rates zero: the rate stays exactly zero
    for k in ("exposure_lr_init", "exposure_lr_final", "exposure_lr_delay_steps", "exposure_lr_delay_mult"):
        setattr(bare, k, 0)
    m3 = _model_with_exposures(["a"], bare)
    m3.update_learning_rate(7)
    assert m3.exposure_optimizer.param_groups[0]["lr"] == 0.0


def test_training_setup_without_exposures_builds_no_exposure_optimizer():
    fx = np.load(FIXTURE)
    opt = fixture_opt(fx)
    assert not any(hasattr(opt, k) for k in ("exposure_lr_init", "exposure_lr_final", "exposure_lr_delay_steps",
                                             "exposure_lr_delay_mult"))
    m = cpu_plain_model(fx)
    assert m.exposure_optimizer is None and m._exposure is None and m.pretrained_exposures is None
    assert m.update_learning_rate(10) is not None                     # nothing to set beside the xyz group
    assert len(m.capture()) == int(fx["capture/length"]) == 12        # today's tuple


def test_setup_exposures_and_lookup_by_name():
    from mvs_gaussian_splatting_amd import GaussianModel
    m = GaussianModel(0)
    with pytest.raises(KeyError, match="IMG_1"):
        m.get_exposure_from_name("IMG_1")
    m.setup_exposures(["IMG_0", "IMG_1", "IMG_2"], device="cpu")
    assert isinstance(m._exposure, torch.nn.Parameter) and m._exposure.shape == (3, 3, 4) and m._exposure.requires_grad
    assert m._exposure.dtype == torch.float32 and m._exposure.is_contiguous()
    assert all(torch.equal(row, torch.eye(3, 4)) for row in m._exposure.detach())
    assert m.exposure_mapping == {"IMG_0": 0, "IMG_1": 1, "IMG_2": 2} and m.pretrained_exposures is None
    row = m.get_exposure_from_name("IMG_1")
    assert row.shape == (3, 4) and row.data_ptr() == m._exposure[1].data_ptr()          # a view: no copy
    (row * torch.arange(12.0).reshape(3, 4)).sum().backward()
    assert torch.equal(m._exposure.grad[1], torch.arange(12.0).reshape(3, 4))            # the gradient lands in the row
    assert not m._exposure.grad[0].any() and not m._exposure.grad[2].any()
    with pytest.raises(KeyError, match="IMG_9"):
        m.get_exposure_from_name("IMG_9")
    with pytest.raises(ValueError, match="distinct"):
        m.setup_exposures(["a", "a"], device="cpu")
    # loaded exposures take over
    m.pretrained_exposures = {"IMG_1": torch.full((3, 4), 2.0)}
    assert torch.equal(m.get_exposure_from_name("IMG_1"), torch.full((3, 4), 2.0))
    with pytest.raises(KeyError, match="IMG_0"):
        m.get_exposure_from_name("IMG_0")


def test_exposure_json_round_trip_is_exact_and_order_free(tmp_path):
    from mvs_gaussian_splatting_amd import load_exposures, save_exposures
    g = torch.Generator().manual_seed(3)
    t = torch.eye(3, 4)[None] + 0.3 * torch.randn(4, 3, 4, generator=g)
    t[0, 0, 0] = 1.0 + 2.0 ** -23                                    # one ulp above 1: must survive the text
    t[1, 2, 3] = 1e-30
    mapping = {"b.png": 2, "a": 0, "view 7": 3, "c": 1}
    path = str(tmp_path / "exposure.json")
    save_exposures(path, mapping, t)
    raw = json.load(open(path))
    assert set(raw) == set(mapping) and all(np.asarray(v).shape == (3, 4) for v in raw.values())   # upstream's format
    back = load_exposures(path)
    assert set(back) == set(mapping)
    for name, idx in mapping.items():
        assert back[name].dtype == torch.float32 and torch.equal(back[name], t[idx]), name
    # the same content written in another key order reads the same
    other = str(tmp_path / "other.json")
    json.dump({k: raw[k] for k in sorted(raw, reverse=True)}, open(other, "w"))
    again = load_exposures(other)
    assert all(torch.equal(again[k], back[k]) for k in back)
    with pytest.raises(ValueError, match="outside"):
        save_exposures(path, {"x": 4}, t)
    json.dump({"x": [[1.0, 0.0], [0.0, 1.0]]}, open(other, "w"))
    with pytest.raises(ValueError, match="3x4"):
        load_exposures(other)


def test_apply_exposure_has_no_cpu_path():
    from mvs_gaussian_splatting_amd import _lib, apply_exposure
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        apply_exposure(torch.rand(3, 5, 7), torch.eye(3, 4))


def test_checkpoint_forms_with_and_without_exposures():
    from mvs_gaussian_splatting_amd import GaussianModel, optim
    fx = np.load(FIXTURE)
    opt = fixture_opt(fx)
    opt.iterations = 100
    plain = cpu_plain_model(fx, optim.Adam)
    cap12 = plain.capture()
    assert len(cap12) == 12
    src = _model_with_exposures(["a", "b"], opt)
    with torch.no_grad():
        src._exposure[1, 0, 3] = 0.25
    src.exposure_optimizer.state[src._exposure] = {"step": torch.tensor(3.0), "exp_avg": torch.full((2, 3, 4), 0.5),
                                                   "exp_avg_sq": torch.full((2, 3, 4), 0.125)}
    cap = src.capture()
    assert len(cap) == 13 and cap[1] is src._xyz
    extra = cap[12]
    assert extra["exposure"] is src._exposure and extra["exposure_mapping"] == {"a": 0, "b": 1}
    assert sorted(extra["exposure_optimizer"]) == ["param_groups", "state"]
    dst = GaussianModel(0)
    dst.setup_exposures(["a", "b"], device="cpu")
    dst.restore(cap, opt, optim.Adam)
    assert dst._exposure is src._exposure and dst.exposure_mapping == {"a": 0, "b": 1}
    st = dst.exposure_optimizer.state[dst._exposure]
    assert float(st["step"]) == 3.0 and torch.equal(st["exp_avg"], torch.full((2, 3, 4), 0.5))
    assert torch.equal(st["exp_avg_sq"], torch.full((2, 3, 4), 0.125))
    assert dst.exposure_optimizer.param_groups[0]["params"][0] is dst._exposure
    # the two sides must agree about having exposures
    with pytest.raises(ValueError, match="exposures"):
        GaussianModel(0).restore(cap, opt, optim.Adam)
    has = GaussianModel(0)
    has.setup_exposures(["a", "b"], device="cpu")
    with pytest.raises(ValueError, match="exposures"):
        has.restore(cap12, opt, optim.Adam)
    # a fork model with exposures: the fork's dict, then the exposures'
    cg = types.SimpleNamespace(learn_split_distance=True, learn_split_scale=False)
    fork = GaussianModel(0, modelcg=cg)
    for a in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        setattr(fork, a, torch.nn.Parameter(getattr(plain, a).detach().clone().requires_grad_(True)))
    fork._split_distance = torch.nn.Parameter(torch.zeros(fork._xyz.shape[0], 3).requires_grad_(True))
    fork.max_radii2D = torch.zeros(fork._xyz.shape[0])
    fork.setup_exposures(["a"], device="cpu")
    fork.training_setup(opt, optim.Adam)
    cap14 = fork.capture()
    assert len(cap14) == 14 and sorted(cap14[12]) == ["_split_distance"] and "exposure_mapping" in cap14[13]
    again = GaussianModel(0, modelcg=cg)
    again.setup_exposures(["a"], device="cpu")
    again.restore(cap14, opt, optim.Adam)
    assert again._split_distance is fork._split_distance and again._exposure is fork._exposure


def test_the_restatement_is_the_matmul_form():
    """The oracle itself against upstream's expression, in float64."""
    g = torch.Generator().manual_seed(0)
    x, gr = torch.rand(3, 5, 7, generator=g), torch.randn(3, 5, 7, generator=g)
    A = (torch.tensor(A_TRUE) + 0.01).double().requires_grad_(True)
    xd = x.double().requires_grad_(True)
    y = torch.matmul(xd.permute(1, 2, 0), A[:3, :3]).permute(2, 0, 1) + A[:3, 3, None, None]
    y.backward(gr.double())
    y64, mag = forward64(x, A)
    dx, dx_mag, dA, dA_mag = backward64(x, A, gr)
    assert (y64 - y.detach()).abs().max() <= 1e-15 and (dx - xd.grad).abs().max() <= 1e-15
    assert (dA - A.grad).abs().max() <= 1e-13
    assert (mag >= y64.abs() - 1e-15).all() and (dx_mag >= dx.abs() - 1e-15).all() and (dA_mag >= dA.abs() - 1e-13).all()
