"""optim.Adam (csrc/adam.hip, gsr_adam_step) against torch.optim.Adam's default (foreach) step on the same GPU: params
and both moments bit-identical (torch.equal) after single and repeated steps, with skipped parameters and per-parameter
step counts, through the optimizer-state surgery of densification, opacity reset and re-layout, through state_dict()
interchange both ways, and over a whole training run."""
import copy
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))

from mvs_gaussian_splatting_amd import optim  # noqa: E402
from mvs_gaussian_splatting_amd.densify import densify_and_prune, FORK_ATTR, FORK_FLAG, GROUP_ATTR  # noqa: E402
from mvs_gaussian_splatting_amd.layout import reorder_gaussians_  # noqa: E402

# arguments/__init__.py:82-107, the reference's defaults
OPT = types.SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016,
                            position_lr_delay_mult=0.01, position_lr_max_steps=30_000, feature_lr=0.0025,
                            opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001, growdirs_lr=0.005,
                            growdistance_lr=0.001, splitdistance_lr=0.005, splitscale_lr=0.005,
                            opacity_reset_interval=3000)
WIDTH = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,),
         "dirs_prob": (128,), "conti_dirs": (3,), "grow_dist": (1,), "split_distance": (3,), "split_scale": (1,)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _model(P, dev, fork=(), seed=0):
    """A duck-typed GaussianModel: the six plain tensors plus the fork's learned tensors of `fork`, as leaves."""
    g = torch.Generator().manual_seed(seed)
    m = types.SimpleNamespace(spatial_lr_scale=2.5, num_dirs=128, modelcg=types.SimpleNamespace())
    for k, a in GROUP_ATTR.items():
        t = torch.randn((P,) + WIDTH[k], generator=g)
        if k == "scaling":
            t = t * 0.5 + torch.log(torch.tensor(0.05))
        setattr(m, a, torch.nn.Parameter(t.to(dev)))
    for k, a in FORK_ATTR.items():
        on = k in fork
        setattr(m, FORK_FLAG[k], on)
        if on:
            setattr(m, a, torch.nn.Parameter(torch.randn((P,) + WIDTH[k], generator=g).to(dev)))
    if "dirs_prob" in fork:
        d = torch.randn(128, 3, generator=g)
        m.dirs = (d / d.norm(dim=1, keepdim=True)).to(dev)
    for f in ("symmetric_split", "split_notreinit", "prob_notreinit"):
        setattr(m.modelcg, f, False)
    m.max_radii2D = torch.zeros(P, device=dev)
    return m


def _clone_model(m):
    c = copy.copy(m)
    for a in list(GROUP_ATTR.values()) + list(FORK_ATTR.values()):
        t = getattr(m, a, None)
        if isinstance(t, torch.Tensor):
            setattr(c, a, torch.nn.Parameter(t.detach().clone()))
    return c


def _grads(model, it, skip=()):
    """Fresh gradients for every group, the same for both runs: normal values with some zero rows and some tiny and
    huge magnitudes; groups in `skip` get grad = None."""
    g = torch.Generator(device=model._xyz.device).manual_seed(1000 + it)
    for grp in model.optimizer.param_groups:
        p = grp["params"][0]
        if grp["name"] in skip:
            p.grad = None
            continue
        x = torch.randn(p.shape, generator=g, device=p.device)
        flat = x.view(-1)
        n = flat.numel()
        flat[0:n:11] = 0.0
        flat[1:n:13] *= 1e-30
        flat[2:n:17] *= 1e15
        flat[3:n:19] *= 1e-7
        p.grad = x


def _assert_same(ma, mb, what):
    oa, ob = ma.optimizer, mb.optimizer
    assert [g["name"] for g in oa.param_groups] == [g["name"] for g in ob.param_groups]
    for ga, gb in zip(oa.param_groups, ob.param_groups):
        pa, pb = ga["params"][0], gb["params"][0]
        assert torch.equal(pa, pb), f"{what}: param {ga['name']} differs"
        sa, sb = oa.state.get(pa, {}), ob.state.get(pb, {})
        assert set(sa) == set(sb), f"{what}: state keys of {ga['name']}"
        for key in ("exp_avg", "exp_avg_sq"):
            if key in sa:
                assert torch.equal(sa[key], sb[key]), f"{what}: {key} of {ga['name']} differs"
        if "step" in sa:
            assert sa["step"].dtype == sb["step"].dtype == torch.float32 and not sb["step"].is_cuda
            assert float(sa["step"]) == float(sb["step"]), f"{what}: step of {ga['name']}"


def _pair(P, dev, fork=(), seed=0):
    a = _model(P, dev, fork, seed)
    b = _clone_model(a)
    optim.training_setup(a, OPT, torch.optim.Adam)
    optim.training_setup(b, OPT, optim.Adam)
    assert isinstance(a.optimizer, torch.optim.Adam) and isinstance(b.optimizer, optim.Adam)
    return a, b


def _step_both(a, b, it, skip=()):
    for m in (a, b):
        _grads(m, it, skip)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)


@pytest.mark.parametrize("P", [1, 7, 4097, 1_000_003])
def test_plain_groups_match_torch_adam(dev, P):
    a, b = _pair(P, dev)
    _step_both(a, b, 0)
    _assert_same(a, b, "one step")
    for it in range(1, 30):
        optim.update_learning_rate(a, it * 500)
        optim.update_learning_rate(b, it * 500)
        _step_both(a, b, it)
    _assert_same(a, b, "30 steps")


def test_unaligned_param_takes_the_scalar_path(dev):
    """A parameter that starts 4 bytes into its storage (and a moment-aligned twin) against torch."""
    base = torch.randn(4 * 4096 + 9, device=dev)
    pa = torch.nn.Parameter(base[1:].clone())
    pb = torch.nn.Parameter(base.clone()[1:])              # a view at a 4-byte offset
    assert pb.data_ptr() % 16 == 4 and pb.is_contiguous()
    oa = torch.optim.Adam([pa], lr=1e-2, eps=1e-15)
    ob = optim.Adam([pb], lr=1e-2, eps=1e-15)
    g = torch.Generator(device=dev).manual_seed(3)
    for _ in range(5):
        gr = torch.randn(pa.shape, generator=g, device=dev)
        pa.grad, pb.grad = gr.clone(), gr.clone()
        oa.step()
        ob.step()
    assert torch.equal(pa, pb)
    assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"])
    assert torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])


def test_fork_groups_with_skipped_params_and_lr_schedule(dev):
    fork = tuple(FORK_ATTR)
    a, b = _pair(5003, dev, fork)
    assert len(b.optimizer.param_groups) == 11
    skips = [(), ("dirs_prob", "grow_dist"), ("split_distance", "split_scale", "conti_dirs"), (), ("dirs_prob",)]
    for it in range(12):
        optim.update_learning_rate(a, 100 * it)
        optim.update_learning_rate(b, 100 * it)
        _step_both(a, b, it, skips[it % len(skips)])
    _assert_same(a, b, "fork groups")
    steps = {g["name"]: float(b.optimizer.state[g["params"][0]]["step"]) for g in b.optimizer.param_groups}
    assert steps["xyz"] == 12 and steps["dirs_prob"] < 12 and len(set(steps.values())) > 1


@torch.no_grad()
def _reset_opacity(m):
    """scene/gaussian_model.py:312-315 with replace_tensor_to_optimizer :386-399 (train.py runs it under no_grad)."""
    opac = torch.sigmoid(m._opacity)
    x = torch.min(opac, torch.ones_like(opac) * 0.01)
    new = torch.log(x / (1 - x))
    for group in m.optimizer.param_groups:
        if group["name"] == "opacity":
            stored = m.optimizer.state.get(group["params"][0], None)
            stored["exp_avg"] = torch.zeros_like(new)
            stored["exp_avg_sq"] = torch.zeros_like(new)
            del m.optimizer.state[group["params"][0]]
            group["params"][0] = torch.nn.Parameter(new.requires_grad_(True))
            m.optimizer.state[group["params"][0]] = stored
            m._opacity = group["params"][0]


@pytest.mark.parametrize("fork", [(), ("dirs_prob", "grow_dist", "split_distance", "split_scale")])
def test_state_surgery_then_continue(dev, fork):
    a, b = _pair(3000, dev, fork, seed=5)
    it = 0
    for phase in ("densify", "reset", "reorder", "densify_again", "end"):
        for _ in range(3):
            _step_both(a, b, it)
            it += 1
        for m in (a, b):
            g = torch.Generator().manual_seed(77 + it)
            P = m._xyz.shape[0]
            m.denom = torch.randint(0, 4, (P, 1), generator=g).float().to(dev)
            m.xyz_gradient_accum = (torch.rand(P, 1, generator=g) * 0.0006).to(dev) * m.denom
            if phase in ("densify", "densify_again"):
                torch.manual_seed(11 + it)                     # the split's (and re-init's) draws, the same for both
                densify_and_prune(m, 0.0002, 0.005, 5.0, 20, opt=OPT, iteration=3100 if phase == "densify" else 1500)
            elif phase == "reset":
                _reset_opacity(m)
            elif phase == "reorder":
                reorder_gaussians_(m)
        _assert_same(a, b, f"after {phase}")
    assert a._xyz.shape[0] != 3000


def test_state_dict_interchange(dev):
    ref, _ = _pair(20000, dev, ("dirs_prob",), seed=9)
    mix = _clone_model(ref)
    optim.training_setup(mix, OPT, torch.optim.Adam)
    # ref: torch all along.  mix: torch, then optim.Adam from torch's state_dict, then torch again from ours
    for it in range(3):
        _step_both(ref, mix, it)
    sd = mix.optimizer.state_dict()
    mix.optimizer = optim.Adam(optim.param_groups(mix, OPT), lr=0.0, eps=1e-15)
    mix.optimizer.load_state_dict(sd)
    for it in range(3, 6):
        _step_both(ref, mix, it, skip=("f_rest",) if it == 4 else ())
    _assert_same(ref, mix, "after torch -> hip")
    sd = mix.optimizer.state_dict()
    mix.optimizer = torch.optim.Adam(optim.param_groups(mix, OPT), lr=0.0, eps=1e-15)
    mix.optimizer.load_state_dict(sd)
    for it in range(6, 9):
        _step_both(ref, mix, it)
    _assert_same(ref, mix, "after hip -> torch")


def test_train_synthetic_hip_optimizer_is_bit_identical(dev):
    from train_synthetic import train
    runs = {}
    for kind in ("torch", "hip"):
        torch.manual_seed(0)
        runs[kind] = train(dev, iterations=60, densification_interval=20, densify_from_iter=10, optimizer=kind)
    (ma, ha, sa), (mb, hb, sb) = runs["torch"], runs["hip"]
    assert isinstance(mb.optimizer, optim.Adam)
    assert ha == hb and sa == sb and len(sa) > 0
    _assert_same(ma, mb, "train_synthetic")
    for a in GROUP_ATTR.values():
        assert torch.equal(getattr(ma, a), getattr(mb, a))


def test_step_on_empty_and_many_tensors(dev):
    """More than one launch's worth of tensors (16 per launch), and empty ones, in one step."""
    ps = [torch.nn.Parameter(torch.randn(n, device=dev)) for n in [0, 5, 4096, 4097, 0] * 5]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    oa, ob = torch.optim.Adam(ps, lr=3e-3, eps=1e-15), optim.Adam(qs, lr=3e-3, eps=1e-15)
    for it in range(3):
        for p, q in zip(ps, qs):
            gr = torch.randn(p.shape, device=dev)
            p.grad, q.grad = gr, gr.clone()
        oa.step()
        ob.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)
        assert float(ob.state[q]["step"]) == 3
