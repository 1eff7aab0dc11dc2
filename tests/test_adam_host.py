"""optim.py without a GPU: the learning-rate schedule and the optimizer table of training_setup against the reference's
own Python (tests/golden/adam_setup.npz, make_golden_adam.py), the per-tensor scalars of a step against the formulas of
torch's _multi_tensor_adam, the options the HIP step does not cover, and the C layout of GsrAdamTensor / GsrAdamBatch."""
import ctypes as C
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

from mvs_gaussian_splatting_amd import _lib, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "adam_setup.npz"))
MODEL_FLAGS = ("grow_dir", "continous_dir", "grow_distance", "learn_split_distance", "learn_split_scale")
FORK_WIDTH = {"dirs_prob": 16, "conti_dirs": 3, "grow_dist": 1, "split_distance": 3, "split_scale": 1}


def _opt():
    names = ("position_lr_init", "position_lr_final", "position_lr_delay_mult", "position_lr_max_steps", "feature_lr",
             "opacity_lr", "scaling_lr", "rotation_lr", "percent_dense", "growdirs_lr", "growdistance_lr",
             "splitdistance_lr", "splitscale_lr")
    o = types.SimpleNamespace(**{k: float(GOLDEN[f"opt/{k}"]) for k in names})
    o.position_lr_max_steps = int(o.position_lr_max_steps)
    return o


def _model(flags, P=10):
    from mvs_gaussian_splatting_amd.densify import FORK_ATTR, FORK_FLAG, GROUP_ATTR
    m = types.SimpleNamespace(spatial_lr_scale=float(GOLDEN["spatial_lr_scale"]))
    shapes = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}
    for k, a in GROUP_ATTR.items():
        setattr(m, a, torch.nn.Parameter(torch.zeros((P,) + shapes[k])))
    for k, a in FORK_ATTR.items():
        on = bool(flags[MODEL_FLAGS.index(FORK_FLAG[k])])
        setattr(m, FORK_FLAG[k], on)
        if on:
            setattr(m, a, torch.nn.Parameter(torch.zeros(P, FORK_WIDTH[k])))
    return m


def test_expon_lr_func_matches_the_reference():
    o = _opt()
    s = float(GOLDEN["spatial_lr_scale"])
    f = optim.expon_lr_func(lr_init=o.position_lr_init * s, lr_final=o.position_lr_final * s,
                            lr_delay_mult=o.position_lr_delay_mult, max_steps=o.position_lr_max_steps)
    got = np.array([f(int(i)) for i in GOLDEN["iters"]], dtype=np.float64)
    assert np.array_equal(got, GOLDEN["lr/default"])
    init, final, steps, mult, max_steps = GOLDEN["lr/delay_args"]
    f = optim.expon_lr_func(lr_init=init, lr_final=final, lr_delay_steps=int(steps), lr_delay_mult=mult,
                            max_steps=int(max_steps))
    got = np.array([f(int(i)) for i in GOLDEN["iters"]], dtype=np.float64)
    assert np.array_equal(got, GOLDEN["lr/delay"])
    assert GOLDEN["lr/delay"][1] < GOLDEN["lr/delay"][20] and GOLDEN["lr/default"][1] > GOLDEN["lr/default"][20]


@pytest.mark.parametrize("case", [str(c) for c in GOLDEN["cases"]])
def test_training_setup_builds_the_reference_optimizer(case):
    m = _model(GOLDEN[f"{case}/flags"])
    opt = optim.training_setup(m, _opt())
    assert opt is m.optimizer and isinstance(opt, optim.Adam) and isinstance(opt, torch.optim.Optimizer)
    groups = opt.param_groups
    assert [g["name"] for g in groups] == list(GOLDEN[f"{case}/names"])
    assert np.array_equal(np.array([g["lr"] for g in groups], dtype=np.float64), GOLDEN[f"{case}/lr"])
    assert np.array_equal(np.array([g["eps"] for g in groups], dtype=np.float64), GOLDEN[f"{case}/eps"])
    assert np.array_equal(np.array([g["betas"] for g in groups], dtype=np.float64), GOLDEN[f"{case}/betas"])
    assert np.array_equal(np.array([g["weight_decay"] for g in groups], dtype=np.float64),
                          GOLDEN[f"{case}/weight_decay"])
    assert [bool(g["amsgrad"]) for g in groups] == list(GOLDEN[f"{case}/amsgrad"])
    assert m.percent_dense == float(GOLDEN[f"{case}/percent_dense"])
    assert tuple(m.xyz_gradient_accum.shape) == tuple(GOLDEN[f"{case}/accum_shape"]) == tuple(m.denom.shape)
    assert not m.xyz_gradient_accum.any() and not m.denom.any()
    updated = np.array([optim.update_learning_rate(m, int(i)) for i in GOLDEN["iters"]], dtype=np.float64)
    assert np.array_equal(updated, GOLDEN[f"{case}/updated_lr"])
    assert groups[0]["lr"] == float(GOLDEN[f"{case}/updated_group_lr"])


def test_training_setup_with_torch_adam_gives_the_same_table():
    m = _model(GOLDEN["grow_dir128/flags"])
    ours = [{k: v for k, v in g.items() if k != "params"} for g in optim.training_setup(m, _opt()).param_groups]
    ref = [{k: v for k, v in g.items() if k != "params"}
           for g in optim.training_setup(m, _opt(), torch.optim.Adam).param_groups]
    assert ours == ref


@pytest.mark.parametrize("lr,betas,eps,step", [(1.6e-4, (0.9, 0.999), 1e-15, 1.0), (0.05, (0.9, 0.999), 1e-15, 7.0),
                                               (2.5e-3, (0.8, 0.99), 1e-8, 12345.0), (0.0, (0.9, 0.999), 1e-15, 3.0),
                                               (1e-3, (0.6, 0.5), 1e-6, 2.0)])
def test_scalars_are_those_of_multi_tensor_adam(lr, betas, eps, step):
    """torch/optim/adam.py _multi_tensor_adam (capturable = False): the lerp weight 1 - beta1, beta2, the addcmul value
    1 - beta2, bias_correction2_sqrt, eps and step_size = (lr / bias_correction1) * -1, in double; then what the
    float fields of GsrAdamTensor hold."""
    beta1, beta2 = betas
    bc1 = [1 - beta1 ** s for s in [step]]
    bc2 = [1 - beta2 ** s for s in [step]]
    want = {"lerp_weight": 1 - beta1, "beta2": beta2, "sq_weight": 1 - beta2, "bc2_sqrt": [b ** 0.5 for b in bc2][0],
            "eps": eps, "step_size": [(lr / b) * -1 for b in bc1][0]}
    got = optim.adam_scalars(lr, betas, eps, step)
    assert got == want and all(type(v) is float for v in got.values())
    t = _lib.GsrAdamTensor()
    for k, v in got.items():
        setattr(t, k, v)
        assert getattr(t, k) == float(np.float32(v))          # the C float: round to nearest, as torch's Scalar.to<float>


def test_step_state_is_torchs():
    """State created lazily and only for params with a grad; the kernel itself needs the GPU."""
    p = torch.nn.Parameter(torch.zeros(4))
    opt = optim.Adam([p], lr=0.1)
    opt.step()                                                # grad is None: skipped, no state
    assert len(opt.state) == 0
    assert opt.state_dict()["param_groups"][0].keys() == torch.optim.Adam([p]).state_dict()["param_groups"][0].keys()


@pytest.mark.parametrize("kw", [dict(weight_decay=0.01), dict(amsgrad=True), dict(maximize=True), dict(capturable=True),
                                dict(differentiable=True), dict(fused=True), dict(decoupled_weight_decay=True)])
def test_unsupported_options_raise(kw):
    with pytest.raises(ValueError):
        optim.Adam([torch.nn.Parameter(torch.zeros(3))], **kw)


def test_bad_params_raise_at_step():
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(_lib.GsrError):                        # CPU: no fallback
        optim.Adam([p]).step()
    opt = optim.Adam([torch.nn.Parameter(torch.zeros(3))])
    opt.param_groups[0]["weight_decay"] = 0.1                 # e.g. from a foreign state_dict
    opt.param_groups[0]["params"][0].grad = torch.ones(3)
    with pytest.raises(ValueError):
        opt.step()


def test_adam_structs_match_the_c_compiler():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "gsr.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(GsrAdamTensor), offsetof(GsrAdamTensor, numel),
         offsetof(GsrAdamTensor, lerp_weight), offsetof(GsrAdamTensor, step_size), offsetof(GsrAdamTensor, exp_avg_sq),
         sizeof(GsrAdamBatch), offsetof(GsrAdamBatch, t), offsetof(GsrAdamBatch, t[1]), GSR_ADAM_MAX_TENSORS);
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = list(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    T, B = _lib.GsrAdamTensor, _lib.GsrAdamBatch
    assert out == [C.sizeof(T), T.numel.offset, T.lerp_weight.offset, T.step_size.offset, T.exp_avg_sq.offset,
                   C.sizeof(B), B.t.offset, B.t.offset + C.sizeof(T), _lib.ADAM_MAX_TENSORS]


def test_adam_step_rejects_bad_batches_before_any_launch():
    lib = _lib.load()
    assert lib.gsr_adam_step(None, None) == -1
    b = _lib.GsrAdamBatch()
    b.count = _lib.ADAM_MAX_TENSORS + 1
    assert lib.gsr_adam_step(C.byref(b), None) == -1
    b.count = -1
    assert lib.gsr_adam_step(C.byref(b), None) == -1
    b.count = 1
    b.t[0].numel = -5
    assert lib.gsr_adam_step(C.byref(b), None) == -1
    b.t[0].numel = 10                                         # NULL arrays of a non-empty entry
    assert lib.gsr_adam_step(C.byref(b), None) == -1
    assert b"NULL" in lib.gsr_last_error()
