"""Generates tests/golden/adam_setup.npz from the reference's own Python (run only where the reference checkout of
make_golden_model.REF exists; the fixture -- plain arrays -- is committed):

    python tests/golden/make_golden_adam.py

1. utils/general_utils.py:29-62 get_expon_lr_func: its values at 40 iterations from -1 to past max_steps, for the
   schedule training_setup builds from the default OptimizationParams (arguments/__init__.py:82-108; no lr_delay_steps,
   so lr_delay_mult has no effect) and for one schedule with delay steps.
2. scene/gaussian_model.py:240-277 training_setup / update_learning_rate: the optimizer's group table (names in order,
   lr, eps, betas, weight_decay, amsgrad), percent_dense and the xyz lr after update_learning_rate, for a plain model and
   for the fork's flag combinations of make_golden_densify_fork.py.  The class is loaded as make_golden_model.py loads it.
"""
import contextlib
import io
import os
import sys
import types
from argparse import ArgumentParser

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_model as mgm  # noqa: E402
from make_golden_densify_fork import ATTR, CASES  # noqa: E402

MODEL_FLAGS = ("grow_dir", "continous_dir", "grow_distance", "learn_split_distance", "learn_split_scale")
WIDTH = {"xyz": (3,), "f_dc": (1, 3), "f_rest": (15, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,),
         "dirs_prob": (16,), "conti_dirs": (3,), "grow_dist": (1,), "split_distance": (3,), "split_scale": (1,)}
FLAG_OF = {"dirs_prob": "grow_dir", "conti_dirs": "continous_dir", "grow_dist": "grow_distance",
           "split_distance": "learn_split_distance", "split_scale": "learn_split_scale"}
SPATIAL_LR_SCALE = 2.5
P = 10
ITERS = np.array([-1, 0, 1, 2, 3, 5, 7, 10, 20, 50, 99, 100, 250, 500, 999, 1000, 1500, 2000, 3000, 4999, 5000, 5001,
                  7000, 7500, 10000, 12345, 15000, 17500, 20000, 22222, 25000, 27000, 29000, 29999, 30000, 30001, 31000,
                  35000, 45000, 100000], dtype=np.int64)
DELAY = dict(lr_init=1e-3, lr_final=1e-5, lr_delay_steps=5000, lr_delay_mult=0.01, max_steps=30000)


def main():
    mod = mgm.load_reference_model_module()               # also puts the reference on sys.path
    from utils.general_utils import get_expon_lr_func
    from arguments import OptimizationParams
    opt = OptimizationParams(ArgumentParser())
    out = {"iters": ITERS, "spatial_lr_scale": np.float64(SPATIAL_LR_SCALE)}
    for k in ("position_lr_init", "position_lr_final", "position_lr_delay_mult", "position_lr_max_steps", "feature_lr",
              "opacity_lr", "scaling_lr", "rotation_lr", "percent_dense", "growdirs_lr", "growdistance_lr",
              "splitdistance_lr", "splitscale_lr"):
        out[f"opt/{k}"] = np.float64(getattr(opt, k))
    f = get_expon_lr_func(lr_init=opt.position_lr_init * SPATIAL_LR_SCALE,
                          lr_final=opt.position_lr_final * SPATIAL_LR_SCALE,
                          lr_delay_mult=opt.position_lr_delay_mult, max_steps=opt.position_lr_max_steps)
    out["lr/default"] = np.array([f(int(i)) for i in ITERS], dtype=np.float64)
    f = get_expon_lr_func(**DELAY)
    out["lr/delay"] = np.array([f(int(i)) for i in ITERS], dtype=np.float64)
    out["lr/delay_args"] = np.array([DELAY[k] for k in ("lr_init", "lr_final", "lr_delay_steps", "lr_delay_mult",
                                                        "max_steps")], dtype=np.float64)

    combos = {"plain": {}}
    for case, (flags, *_rest) in CASES.items():
        key = tuple(bool(flags.get(f, False)) for f in MODEL_FLAGS)
        if key not in [tuple(bool(c.get(f, False)) for f in MODEL_FLAGS) for c in combos.values()]:
            combos[case] = {f: True for f in MODEL_FLAGS if flags.get(f)}
    g = torch.Generator().manual_seed(0)
    for case, flags in combos.items():
        cg = types.SimpleNamespace(learn_split_distance=bool(flags.get("learn_split_distance")),
                                   learn_split_scale=bool(flags.get("learn_split_scale")), symmetric_split=False,
                                   split_notreinit=False, prob_notreinit=False)
        with mgm._Patched():
            m = mod.GaussianModel(3, grow_dir=bool(flags.get("grow_dir")), num_dirs=16,
                                  continous_dir=bool(flags.get("continous_dir")),
                                  grow_distance=bool(flags.get("grow_distance")), modelcg=cg)
        for k, w in WIDTH.items():
            if k in FLAG_OF and not flags.get(FLAG_OF[k]):
                continue
            setattr(m, ATTR[k], torch.nn.Parameter(torch.randn((P,) + w, generator=g)))
        m.spatial_lr_scale = SPATIAL_LR_SCALE
        with mgm._Patched(), contextlib.redirect_stdout(io.StringIO()):
            m.training_setup(opt)
        groups = m.optimizer.param_groups
        out[f"{case}/flags"] = np.array([bool(flags.get(f, False)) for f in MODEL_FLAGS])
        out[f"{case}/names"] = np.array([grp["name"] for grp in groups])
        out[f"{case}/lr"] = np.array([grp["lr"] for grp in groups], dtype=np.float64)
        out[f"{case}/eps"] = np.array([grp["eps"] for grp in groups], dtype=np.float64)
        out[f"{case}/betas"] = np.array([grp["betas"] for grp in groups], dtype=np.float64)
        out[f"{case}/weight_decay"] = np.array([grp["weight_decay"] for grp in groups], dtype=np.float64)
        out[f"{case}/amsgrad"] = np.array([grp["amsgrad"] for grp in groups])
        out[f"{case}/percent_dense"] = np.float64(m.percent_dense)
        out[f"{case}/accum_shape"] = np.array(m.xyz_gradient_accum.shape)
        out[f"{case}/updated_lr"] = np.array([m.update_learning_rate(int(i)) for i in ITERS], dtype=np.float64)
        out[f"{case}/updated_group_lr"] = np.float64(m.optimizer.param_groups[0]["lr"])
    out["cases"] = np.array(list(combos))
    path = os.path.join(HERE, "adam_setup.npz")
    np.savez(path, **out)
    print("wrote", path, "cases:", list(combos))


if __name__ == "__main__":
    main()
