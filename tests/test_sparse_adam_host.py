"""optim.SparseGaussianAdam without a GPU: ABI 21 and the C layout of GsrAdamRowsBatch, the argument checks of
gsr_adam_step_rows, OptimizationParams.optimizer_type and the class training_setup builds from it, and the checks of
step(visibility) that run before the device is needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile
import types

import pytest
import torch

from mvs_gaussian_splatting_amd import _lib, optim
from mvs_gaussian_splatting_amd.densify import GROUP_ATTR
from mvs_gaussian_splatting_amd.trainer import OptimizationParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}


def _model(P=10):
    m = types.SimpleNamespace(spatial_lr_scale=2.5)
    for k, a in GROUP_ATTR.items():
        setattr(m, a, torch.nn.Parameter(torch.zeros((P,) + SHAPES[k])))
    for flag in ("grow_dir", "continous_dir", "grow_distance", "learn_split_distance", "learn_split_scale"):
        setattr(m, flag, False)
    return m


def test_abi_version_is_21_everywhere():
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    lib = _lib.load()
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 21
    assert hasattr(lib, "gsr_adam_step_rows")


def test_rows_batch_matches_the_c_compiler_and_the_old_structs_keep_their_size():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "gsr.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %d %d %zu %zu\n", sizeof(GsrAdamRowsBatch), offsetof(GsrAdamRowsBatch, visibility),
         offsetof(GsrAdamRowsBatch, rows), offsetof(GsrAdamRowsBatch, visibility_kind), offsetof(GsrAdamRowsBatch, count),
         offsetof(GsrAdamRowsBatch, t), offsetof(GsrAdamRowsBatch, t[1]), GSR_ADAM_VIS_U8, GSR_ADAM_VIS_I32,
         sizeof(GsrAdamTensor), sizeof(GsrAdamBatch));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = list(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    R, T, B = _lib.GsrAdamRowsBatch, _lib.GsrAdamTensor, _lib.GsrAdamBatch
    assert out == [C.sizeof(R), R.visibility.offset, R.rows.offset, R.visibility_kind.offset, R.count.offset, R.t.offset,
                   R.t.offset + C.sizeof(T), _lib.ADAM_VIS_U8, _lib.ADAM_VIS_I32, C.sizeof(T), C.sizeof(B)]
    assert (C.sizeof(T), C.sizeof(B)) == (64, 8 + 16 * 64)       # what ABI 16 shipped


def test_adam_step_rows_rejects_bad_batches_before_any_launch():
    lib = _lib.load()
    assert lib.gsr_adam_step_rows(None, None) == -1
    b = _lib.GsrAdamRowsBatch()
    b.count = _lib.ADAM_MAX_TENSORS + 1
    assert lib.gsr_adam_step_rows(C.byref(b), None) == -1
    b.count = -1
    assert lib.gsr_adam_step_rows(C.byref(b), None) == -1
    b.count = 1
    b.visibility_kind = 2
    assert lib.gsr_adam_step_rows(C.byref(b), None) == -1 and b"visibility_kind" in lib.gsr_last_error()
    b.visibility_kind = _lib.ADAM_VIS_I32
    b.t[0].numel = -5
    assert lib.gsr_adam_step_rows(C.byref(b), None) == -1
    b.t[0].numel = 12
    b.rows = 4
    assert lib.gsr_adam_step_rows(C.byref(b), None) == -1 and b"NULL param" in lib.gsr_last_error()
    buf = (C.c_float * 64)()
    for f in ("param", "grad", "exp_avg", "exp_avg_sq"):
        setattr(b.t[0], f, C.addressof(buf))
    assert lib.gsr_adam_step_rows(C.byref(b), None) == -1 and b"NULL visibility" in lib.gsr_last_error()
    b.visibility = C.addressof(buf)
    b.rows = 5                                                 # 12 floats in 5 rows
    assert lib.gsr_adam_step_rows(C.byref(b), None) == -1 and b"multiple of rows" in lib.gsr_last_error()
    b.rows = 0
    assert lib.gsr_adam_step_rows(C.byref(b), None) == -1
    b.rows = -4
    assert lib.gsr_adam_step_rows(C.byref(b), None) == -1
    b.rows = 4
    b.visibility = C.addressof(buf) + 1                        # int32 entries at an odd address
    assert lib.gsr_adam_step_rows(C.byref(b), None) == -3


def test_optimizer_type_defaults_to_default():
    assert OptimizationParams().optimizer_type == "default"
    assert OptimizationParams(optimizer_type="sparse_adam").optimizer_type == "sparse_adam"


def test_training_setup_picks_the_class_from_optimizer_type():
    dense = optim.training_setup(_model(), OptimizationParams())
    sparse = optim.training_setup(_model(), OptimizationParams(optimizer_type="sparse_adam"))
    assert type(dense) is optim.Adam and type(sparse) is optim.SparseGaussianAdam and isinstance(sparse, optim.Adam)
    strip = lambda o: [{k: v for k, v in g.items() if k != "params"} for g in o.param_groups]   # noqa: E731
    assert strip(dense) == strip(sparse)
    assert [g["name"] for g in sparse.param_groups] == list(GROUP_ATTR)
    assert all(g["eps"] == 1e-15 for g in sparse.param_groups)
    # an explicit class wins over the field
    assert type(optim.training_setup(_model(), OptimizationParams(optimizer_type="sparse_adam"), torch.optim.Adam)) \
        is torch.optim.Adam
    with pytest.raises(ValueError):
        optim.training_setup(_model(), OptimizationParams(optimizer_type="sparse"))


def test_gaussian_model_training_setup_and_restore_follow_optimizer_type():
    from mvs_gaussian_splatting_amd import GaussianModel
    m = GaussianModel(1)
    for k, a in GROUP_ATTR.items():
        setattr(m, a, torch.nn.Parameter(torch.zeros((6,) + SHAPES[k])))
    opt = OptimizationParams(optimizer_type="sparse_adam")
    assert type(m.training_setup(opt)) is optim.SparseGaussianAdam
    saved = m.capture()
    m2 = GaussianModel(1)
    m2.restore(saved, opt)
    assert type(m2.optimizer) is optim.SparseGaussianAdam
    m2.restore(saved, OptimizationParams())
    assert type(m2.optimizer) is optim.Adam
    with pytest.raises(ValueError):
        m2.training_setup(OptimizationParams(optimizer_type="fused"))


def test_step_checks_the_visibility_before_any_state_changes():
    P = 6
    ps = [torch.nn.Parameter(torch.zeros(P, 3)), torch.nn.Parameter(torch.zeros(P, 1))]
    opt = optim.SparseGaussianAdam([{"params": [p], "name": n} for p, n in zip(ps, ("xyz", "opacity"))], lr=0.1)
    opt.step(torch.ones(P + 1, dtype=torch.bool))             # no gradients: nothing is checked, nothing happens
    assert len(opt.state) == 0
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(ValueError):
        opt.step(torch.ones(P + 1, dtype=torch.bool))          # wrong length
    with pytest.raises(ValueError):
        opt.step(torch.ones(P, 1, dtype=torch.bool))           # not [P]
    with pytest.raises(ValueError):
        opt.step(torch.ones(2 * P, dtype=torch.int32)[::2])    # not contiguous
    for dtype in (torch.float32, torch.float64, torch.int64):
        with pytest.raises(TypeError):
            opt.step(torch.ones(P, dtype=dtype))
    with pytest.raises(TypeError):
        opt.step([True] * P)
    assert len(opt.state) == 0
    for dtype in (torch.bool, torch.uint8, torch.int32):      # well-formed: as far as the device check, no CPU path
        with pytest.raises(_lib.GsrError):
            opt.step(torch.ones(P, dtype=dtype))
    with pytest.raises(_lib.GsrError):
        opt.step()                                             # visibility=None is Adam.step()
    assert len(opt.state) == 0
    # a parameter of another height is an error unless its group is stepped densely
    ps[1].grad = None
    ps.append(torch.nn.Parameter(torch.zeros(P + 2, 3)))
    opt.add_param_group({"params": [ps[2]], "name": "other"})
    ps[2].grad = torch.ones_like(ps[2])
    with pytest.raises(ValueError):
        opt.step(torch.ones(P, dtype=torch.bool))
    with pytest.raises(_lib.GsrError):
        opt.step(torch.ones(P, dtype=torch.bool), dense=("other",))
    assert len(opt.state) == 0
