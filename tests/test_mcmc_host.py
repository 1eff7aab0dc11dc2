"""MCMC densification, the part that runs without a GPU: the ABI surface (v25), argument refusal before any device use,
the restatement (tests/mcmc_restate.py) against independent evaluations, and the trainer's argument checks for
``strategy="mcmc"``.  The kernels are checked in tests/test_gpu_mcmc.py."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import mcmc_restate as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gsr_mcmc_noise", "gsr_mcmc_reg_workspace_bytes", "gsr_mcmc_reg_fwd", "gsr_mcmc_reg_bwd",
               "gsr_mcmc_sample_workspace_bytes", "gsr_mcmc_sample", "gsr_mcmc_relocation")
BADARG, ALIGN = -1, -3


def test_entry_points_are_exported_and_the_three_abi_numbers_agree():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.SYMBOLS and re.search(rf"\b{name}\s*\(", header), name
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 25


def test_the_makefile_builds_the_unit_without_contraction():
    mk = open(os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS = .*\bmcmc\.o\b", mk, re.M)
    assert re.search(r"^CONTRACT_OFF_OBJS :?\+?= *mcmc\.o\b", mk, re.M)
    flags = re.search(r"^\$\(CONTRACT_OFF_OBJS\): (\w+) \+= -ffp-contract=off$", mk, re.M)
    assert flags and re.search(r"^%\.o: %\.hip.*\n\t.*\$\(" + flags.group(1) + r"\)", mk, re.M)


def test_every_entry_point_refuses_bad_arguments_without_a_device():
    """NULL, negative and too-small arguments come back as GSR_E_BADARG (misaligned ones as GSR_E_ALIGN) before any HIP
    call -- this machine has no device to call -- and an empty problem returns 0 without a launch.  The non-NULL
    pointers are host buffers: they are only looked at as addresses."""
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)                       # 16-byte aligned host memory
    assert p % 16 == 0
    big = 1 << 40
    # noise
    assert lib.gsr_mcmc_noise(4, None, p, p, p, p, 1.0, None) == BADARG
    assert lib.gsr_mcmc_noise(4, p, p, p, p, None, 1.0, None) == BADARG
    assert lib.gsr_mcmc_noise(-1, p, p, p, p, p, 1.0, None) == BADARG
    assert lib.gsr_mcmc_noise(1 << 31, p, p, p, p, p, 1.0, None) == BADARG
    assert lib.gsr_mcmc_noise(4, p, p, p + 4, p, p, 1.0, None) == ALIGN and b"16-byte" in lib.gsr_last_error()
    assert lib.gsr_mcmc_noise(4, p + 2, p, p, p, p, 1.0, None) == ALIGN
    assert lib.gsr_mcmc_noise(0, None, None, None, None, None, 1.0, None) == 0
    # priors
    need = lib.gsr_mcmc_reg_workspace_bytes()
    assert need >= 2 * 8 and need % 8 == 0
    assert lib.gsr_mcmc_reg_fwd(None, p, 4, 0.01, 0.01, p, p, big, None) == BADARG
    assert lib.gsr_mcmc_reg_fwd(p, p, 4, 0.01, 0.01, None, p, big, None) == BADARG
    assert lib.gsr_mcmc_reg_fwd(p, p, 4, 0.01, 0.01, p, None, big, None) == BADARG
    assert lib.gsr_mcmc_reg_fwd(p, p, -1, 0.01, 0.01, p, p, big, None) == BADARG
    assert lib.gsr_mcmc_reg_fwd(p, p, 4, 0.01, 0.01, p, p, need - 1, None) == BADARG and b"workspace" in lib.gsr_last_error()
    assert lib.gsr_mcmc_reg_fwd(p, p, 4, 0.01, 0.01, p + 8, p, big, None) == ALIGN
    assert lib.gsr_mcmc_reg_fwd(None, None, 0, 0.01, 0.01, p, p, big, None) == 0
    assert lib.gsr_mcmc_reg_bwd(p, p, 4, None, p, p, p, None) == BADARG
    assert lib.gsr_mcmc_reg_bwd(p, p, 4, p, None, p, p, None) == BADARG
    assert lib.gsr_mcmc_reg_bwd(p, p, 4, p, p, None, p, None) == BADARG
    assert lib.gsr_mcmc_reg_bwd(p, p, -3, p, p, p, p, None) == BADARG
    assert lib.gsr_mcmc_reg_bwd(None, None, 0, p, p, None, None, None) == 0
    # sampler
    assert lib.gsr_mcmc_sample_workspace_bytes(-1) == 0 == lib.gsr_mcmc_sample_workspace_bytes(1 << 31)
    w1, w2 = lib.gsr_mcmc_sample_workspace_bytes(1000), lib.gsr_mcmc_sample_workspace_bytes(6_000_000)
    assert w1 >= 8 * 1001 and 8 * 6_000_000 < w2 < 9 * 6_000_000
    assert lib.gsr_mcmc_sample(4, None, 0.005, p, 2, p, p, p, big, None) == BADARG
    assert lib.gsr_mcmc_sample(4, p, 0.005, None, 2, p, p, p, big, None) == BADARG
    assert lib.gsr_mcmc_sample(4, p, 0.005, p, 2, None, p, p, big, None) == BADARG
    assert lib.gsr_mcmc_sample(4, p, 0.005, p, 2, p, None, p, big, None) == BADARG
    assert lib.gsr_mcmc_sample(4, p, 0.005, p, 2, p, p, None, big, None) == BADARG
    assert lib.gsr_mcmc_sample(-1, p, 0.005, p, 2, p, p, p, big, None) == BADARG
    assert lib.gsr_mcmc_sample(4, p, 0.005, p, -2, p, p, p, big, None) == BADARG
    assert lib.gsr_mcmc_sample(0, None, 0.005, p, 2, p, None, None, 0, None) == BADARG      # samples of nothing
    assert lib.gsr_mcmc_sample(1000, p, 0.005, p, 2, p, p, p, w1 - 1, None) == BADARG and b"workspace" in lib.gsr_last_error()
    assert lib.gsr_mcmc_sample(4, p, 0.005, p + 4, 2, p, p, p, big, None) == ALIGN
    assert lib.gsr_mcmc_sample(0, None, 0.005, None, 0, None, None, None, 0, None) == 0
    # relocation
    for hole in range(6):
        args = [p] * 6
        args[hole] = None
        assert lib.gsr_mcmc_relocation(3, *args, None) == BADARG, hole
    assert lib.gsr_mcmc_relocation(-1, p, p, p, p, p, p, None) == BADARG
    assert lib.gsr_mcmc_relocation(3, p + 1, p, p, p, p, p, None) == ALIGN
    assert lib.gsr_mcmc_relocation(0, None, None, None, None, None, None, None) == 0


# ---- the restatement against independent evaluations ---------------------------------------------------------------
def test_relocation_with_one_copy_is_the_identity():
    for o32 in (np.float32(0.006), np.float32(0.5), np.float32(0.99), np.float32(0.123456)):
        s = np.array([0.03, 1.7, 0.0004], dtype=np.float32).astype(np.float64)
        op, D, sp, _, new_s = rs.relocation64(float(o32), s, 1)
        assert op == float(o32) and D == float(o32)
        assert np.array_equal(sp, s) and np.array_equal(new_s, np.log(s))


@pytest.mark.parametrize("N", [2, 3, 51])
@pytest.mark.parametrize("o", [0.006, 0.5, 0.99])
def test_relocation_keeps_the_covered_area(o, N):
    """What the correction is built on: N copies of opacity o' and scale s' composited over each other cover, along a line
    through the centre, what the one Gaussian of opacity o and scale s covered:
        integral 1 - (1 - o' g_s'(x))^N dx  =  integral o g_s(x) dx  =  o s sqrt(2 pi),   g_s(x) = exp(-x^2 / (2 s^2)).
    The left side is integrated numerically (no binomials), to 1e-12."""
    s = 0.37
    op, D, sp, _, _ = rs.relocation64(o, s, N)
    assert 0.0 < op < o and float(sp) > 0.0
    lhs = rs.coverage_quadrature(op, float(sp), N)
    rhs = o * s * math.sqrt(2.0 * math.pi)
    # the rule itself, on the integral it can be checked on in closed form
    assert abs(rs.coverage_quadrature(o, s, 1) - rhs) <= 1e-13 * rhs
    assert abs(lhs - rhs) <= 1e-12 * rhs, (lhs, rhs, (lhs - rhs) / rhs)
    # counts above 51 are clamped
    assert rs.relocation64(o, s, 500)[:2] == rs.relocation64(o, s, 51)[:2]


def test_sampled_indices_are_searchsorted_right():
    g = np.random.default_rng(5)
    o = g.random(700).astype(np.float32)
    o[100:164] = 0.001                         # a dead run
    o[:3] = 0.0
    o[-2:] = 0.004
    w = rs.weights(o, 0.005)
    assert all(wi == 0 for wi in w[100:164]) and w[0] == 0 and w[-1] == 0 and w[5] == int(round(float(o[5]) * 2 ** 30))
    draws = [int(x) for x in g.integers(0, 2 ** 63, size=4000, dtype=np.int64)] + rs.edge_draws(w)
    idx, count, Cs = rs.sample(w, draws)
    T = Cs[-1]
    ts = [(r * T) >> 63 for r in draws]
    assert max(ts) == T - 1 and min(ts) == 0
    want = np.searchsorted(np.array(Cs, dtype=np.int64), np.array(ts, dtype=np.int64), side="right")
    assert np.array_equal(np.array(idx), want)
    assert sum(count) == len(draws) and all(w[i] > 0 for i in idx)
    assert [count[i] for i in range(len(w))] == np.bincount(want, minlength=len(w)).tolist()
    # every row (alive_threshold < 0) and no row
    assert all(wi > 0 for wi in rs.weights(o[3:], -1.0))
    assert rs.sample([0, 0, 0], [1, 2 ** 62]) == ([-1, -1], [0, 0, 0], [0, 0, 0])


def test_noise_restatement_is_the_covariance_product():
    """delta = Sigma v with Sigma = R diag(s^2) R^T formed the long way; the magnitudes bound it."""
    g = torch.Generator().manual_seed(2)
    P = 50
    sc, rot = 0.5 * torch.randn(P, 3, generator=g) - 3.0, torch.randn(P, 4, generator=g)
    op, nz = 3.0 * torch.randn(P, 1, generator=g) - 4.0, torch.randn(P, 3, generator=g)
    out = rs.noise64(sc.numpy(), rot.numpy(), op.numpy(), nz.numpy(), 0.37)
    q = torch.nn.functional.normalize(rot.double())
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    L = R * torch.exp(sc.double())[:, None, :]
    cov = L @ L.transpose(1, 2)
    o = torch.sigmoid(op.double())
    v = nz.double() * torch.sigmoid(100.0 * ((1 - o) - 0.995)) * float(np.float32(0.37))
    want = torch.bmm(cov, v[:, :, None])[:, :, 0].numpy()
    assert np.abs(out["delta"] - want).max() <= 1e-14 * np.abs(want).max()
    assert (out["mag"] >= np.abs(out["delta"]) * (1 - 1e-12)).all() and (out["mag_rot"] >= 2 * out["mag"] * (1 - 1e-12)).all()


def test_reg_restatement_is_the_torch_composition():
    g = torch.Generator().manual_seed(4)
    op = torch.randn(33, 1, generator=g).double().requires_grad_(True)
    sc = (torch.randn(33, 3, generator=g) - 2.0).double().requires_grad_(True)
    wo, ws = float(np.float32(0.01)), float(np.float32(0.02))
    val = wo * torch.sigmoid(op).mean() + ws * torch.exp(sc).mean()
    val.backward()
    value, go, gs, _ = rs.reg64(op.detach().numpy(), sc.detach().numpy(), 0.01, 0.02)
    assert abs(value - float(val.detach())) <= 1e-15
    assert np.abs(go - op.grad.numpy()).max() <= 1e-18 and np.abs(gs - sc.grad.numpy()).max() <= 1e-18


# ---- trainer: the checks trip before any device use ----------------------------------------------------------------
def test_optimization_params_defaults_leave_everything_as_it_is():
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams
    o = OptimizationParams()
    assert (o.strategy, o.cap_max, o.noise_lr, o.opacity_reg, o.scale_reg) == ("default", -1, 5e5, 0.01, 0.01)
    assert OptimizationParams(strategy="mcmc", cap_max=1000).cap_max == 1000


def _cpu_model(fork=False):
    m = types.SimpleNamespace()
    m._xyz = torch.zeros(5, 3)
    if fork:
        m.grow_dir = True
    return m


def test_training_iteration_validates_the_mcmc_arguments_before_touching_the_device():
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, schedule
    opt = OptimizationParams(strategy="mcmc", densify_from_iter=10, densification_interval=10, densify_until_iter=50)
    # the schedule is the default strategy's: relocation and growth fire where densify_and_prune would
    assert [i for i in range(1, 60) if schedule(opt, i)["densify"]] == [20, 30, 40]
    call = lambda model, o, **kw: trainer.training_iteration(model, None, o, None, None, 1, cameras_extent=1.0, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="cap_max"):
        call(_cpu_model(), opt)                                                     # cap_max = -1
    with pytest.raises(ValueError, match="cap_max"):
        call(_cpu_model(), OptimizationParams(strategy="mcmc", cap_max=0))
    with pytest.raises(ValueError, match="fork"):
        call(_cpu_model(fork=True), OptimizationParams(strategy="mcmc", cap_max=100))
    with pytest.raises(ValueError, match="unknown keys"):
        call(_cpu_model(), OptimizationParams(strategy="mcmc", cap_max=100), mcmc_kwargs={"seed": 1})
    with pytest.raises(ValueError, match="strategy"):
        call(_cpu_model(), OptimizationParams(strategy="annealing", cap_max=100))
    with pytest.raises(ValueError, match="mcmc_kwargs"):
        call(_cpu_model(), OptimizationParams(), mcmc_kwargs={})


def test_the_strategy_functions_refuse_fork_models_and_cpu_tensors():
    from mvs_gaussian_splatting_amd import _lib, add_new_gs, inject_noise, mcmc_regularizer, relocate_gs
    from mvs_gaussian_splatting_amd.synthetic import SyntheticGaussianModel
    fork = SyntheticGaussianModel(8, 0)
    fork.continous_dir = True
    for fn in (lambda: relocate_gs(fork), lambda: add_new_gs(fork, 100), lambda: inject_noise(fork, 1.0)):
        with pytest.raises(ValueError, match="fork"):
            fn()
    plain = SyntheticGaussianModel(8, 0)
    for fn in (lambda: relocate_gs(plain), lambda: add_new_gs(plain, 100), lambda: inject_noise(plain, 1.0),
               lambda: mcmc_regularizer(plain._opacity, plain._scaling, 0.01, 0.01)):
        with pytest.raises(_lib.GsrError, match="no CPU path"):
            fn()
