"""Host side of the fork's grow / learned-split branch (gaussian_renderer/__init__.py:91-253): the gate predicate
against every boundary of :92-93 and :186, and a float64 restatement of the branch (tests/grow_restate.py) against the
fixture recorded from the reference's own render() (tests/golden/make_golden_grow.py)."""
import os
import types

import numpy as np
import pytest
import torch

from grow_restate import RECORDED, case_config, case_model, cotangent, restate, selection
from mvs_gaussian_splatting_amd import grow

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grow_branch.npz")
OPT = types.SimpleNamespace(densify_from_iter=500, densification_interval=100, densify_until_iter=15000,
                            opacity_reset_interval=3000)


def cg(d=False, s=False):
    return types.SimpleNamespace(learn_split_distance=d, learn_split_scale=s)


# (iteration, opt, grow_dir, continous_dir, modelcg, expected)
GATE = [
    (None, OPT, True, False, cg(True, True), None),              # :91 no iteration (training_report)
    (4000, None, True, False, cg(True, True), None),             # :91 no opt
    (4000, OPT, False, False, None, None),                       # no flag at all
    (4000, OPT, False, False, cg(), None),
    (4000, OPT, True, False, None, "grow"),
    (4000, OPT, False, True, None, "grow"),
    (4000, OPT, True, True, None, "grow"),
    # :92 window 500 - 100 - 1 = 399 < it < 15000
    (399, OPT, True, False, None, None),
    (400, OPT, True, False, None, None),                         # inside the window, before the reset (:93)
    (14999, OPT, True, False, None, "grow"),
    (15000, OPT, True, False, None, None),
    # :93 it > opacity_reset_interval
    (3000, OPT, True, False, None, None),
    (3001, OPT, True, False, None, "grow"),
    # inside the window with the inner test failing: plain, the learned split is NOT tried
    (3000, OPT, True, False, cg(True, True), None),
    (400, OPT, False, True, cg(True, False), None),
    # outside the window: the elif of :186 takes over when a split flag is set
    (399, OPT, True, False, cg(True, False), "split"),
    (15000, OPT, True, False, cg(False, True), "split"),
    (399, OPT, True, False, None, None),
    # :186 the learned split has no iteration window
    (0, OPT, False, False, cg(True, False), "split"),
    (1, OPT, False, False, cg(False, True), "split"),
    (10 ** 6, OPT, False, False, cg(True, True), "split"),
    (4000, OPT, False, False, cg(True, True), "split"),
    (4000, OPT, True, False, cg(True, True), "grow"),            # grow wins inside its window
]


@pytest.mark.parametrize("it,opt,gd,cd,mcg,want", GATE)
def test_gate_predicate(it, opt, gd, cd, mcg, want):
    assert grow.branch(it, opt, gd, cd, mcg) == want


def test_mode_bits():
    assert grow.mode_bits("grow", grow_dir=True) == 1
    assert grow.mode_bits("grow", grow_dir=True, continous_dir=True, grow_distance=True) == 1 | 4    # :98 if / elif
    assert grow.mode_bits("grow", continous_dir=True, grow_distance=True) == 2 | 4
    assert grow.mode_bits("split", modelcg=cg(True, False)) == 8
    assert grow.mode_bits("split", modelcg=cg(True, True)) == 8 | 16


def test_percent_dense_extent():
    pc = types.SimpleNamespace(percent_dense=0.01)
    assert grow.percent_dense_extent(pc, "grow", None, None) == float("inf")
    assert grow.percent_dense_extent(pc, "split", cg(True), 5.0) == float(np.float32(0.05))
    with pytest.raises(ValueError, match="cameras_extent"):
        grow.percent_dense_extent(pc, "split", cg(True), None)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _cases(z, raises=False):
    return [str(n) for n in z["cases"] if bool(z[f"{n}/raises"]) == raises]


def test_fixture_shape(golden):
    z = golden
    assert os.path.getsize(GOLDEN) < 1_000_000
    assert list(_cases(z, True)) == ["grow_split_raises"]
    P = z["model/xyz"].shape[0]
    assert P == 128 and z["model/dirs_prob"].shape == (128, 128) and z["model/f_rest"].shape[1] == 15
    assert bool(z["gate_inner_closed/selected_is_none"])


def test_gate_agrees_with_the_fixture(golden):
    z = golden
    opt = types.SimpleNamespace(**dict(zip(("densify_from_iter", "densification_interval", "densify_until_iter",
                                            "opacity_reset_interval"), (int(v) for v in z["opt"]))))
    for name in _cases(z):
        which, flags, _, _ = case_config(z, name)
        got = grow.branch(int(z[f"{name}/arg/iteration"]), opt, flags["grow_dir"], flags["continous_dir"],
                          cg(flags["learn_split_distance"], flags["learn_split_scale"]))
        P = z["model/xyz"].shape[0]
        grown = z[f"{name}/ext/means3D"].shape[0] > P or not bool(z[f"{name}/selected_is_none"])
        assert (got is not None) == grown, name
        if got is not None:
            assert got == which, name


@pytest.mark.parametrize("name", ["grow_dir", "grow_dir_distance", "continous_dir", "split_distance", "split_scale",
                                  "split_both", "grow_split_zero"])
def test_restatement_reproduces_the_reference(golden, name):
    z = golden
    which, flags, thr, pde = case_config(z, name)
    m = case_model(z)
    P = m["xyz"].shape[0]
    m2 = torch.zeros(P, 3, dtype=torch.float64, requires_grad=True)
    noise = torch.from_numpy(z[f"{name}/noise"]).double()
    ext, sel = restate(m, which, flags, thr, pde, m2, noise)
    assert torch.equal(sel, torch.from_numpy(z[f"{name}/selected"]))
    G = int(sel.sum())
    assert G > 20 and z[f"{name}/ext/means3D"].shape[0] == P + G
    assert z[f"{name}/radii"].shape == (P,)
    for k in RECORDED:
        ref = torch.from_numpy(z[f"{name}/ext/{k}"]).double()
        got = ext[k].detach()
        assert got.shape == ref.shape, k
        err = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
        assert err < 2e-6, f"{name}: {k} differs by {err:.2e}"
    w = cotangent(int(z[f"{name}/cotangent_seed"]), {k: ext[k].shape for k in RECORDED})
    sum((w[k].double() * ext[k]).sum() for k in RECORDED).backward()
    none = set(str(s) for s in z[f"{name}/grad_none"])
    for k in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "dirs_prob", "conti_dirs", "grow_dist",
              "split_distance", "split_scale"):
        g = m[k].grad
        if k in none:
            assert g is None, f"{name}: {k} must get no gradient"
            continue
        ref = torch.from_numpy(z[f"{name}/grad/{k}"]).double()
        assert g is not None, f"{name}: {k} has no gradient"
        scale = float(ref.abs().max())
        err = float((g - ref).abs().max()) / scale if scale > 0 else float(g.abs().max())
        assert err < 1e-5, f"{name}: grad {k} differs by {err:.2e}"
    ref = torch.from_numpy(z[f"{name}/grad/means2D"]).double()
    assert float((m2.grad - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_the_raising_case_is_a_grow_frame_with_split_rows(golden):
    z = golden
    m = case_model(z)
    for name, want in (("grow_split_raises", True), ("grow_split_zero", False)):
        which, flags, thr, pde = case_config(z, name) if name != "grow_split_raises" else (
            "grow", None, float(z["threshold"]), float(np.float32(float(z["percent_dense"]) *
                                                                   float(z[f"{name}/extent"]))))
        sel, big = selection(m, "grow", thr, pde)
        assert bool((sel & big).any()) == want, name


def test_grow_struct_layouts_match_the_c_compiler(tmp_path):
    """GsrGrow / GsrGrowGrads (include/gsr.h, ABI v14) as ctypes lays them out."""
    import ctypes as C
    import subprocess
    from mvs_gaussian_splatting_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "gsr.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(GsrGrow), sizeof(GsrGrowGrads), offsetof(GsrGrow, xyz),
         offsetof(GsrGrow, noise), offsetof(GsrGrow, src), offsetof(GsrGrowGrads, out), offsetof(GsrGrowGrads, d_dirs_prob),
         offsetof(GsrGrowGrads, d_split_scale), GSR_GROW_CONTINUOUS, GSR_SPLIT_SCALE);
  return 0;
}'''
    c = tmp_path / "t.c"
    c.write_text(prog)
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(c), "-o", str(exe)], check=True)
    vals = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    G, D = _lib.GsrGrow, _lib.GsrGrowGrads
    assert vals == [C.sizeof(G), C.sizeof(D), G.xyz.offset, G.noise.offset, G.src.offset, D.out.offset,
                    D.d_dirs_prob.offset, D.d_split_scale.offset, _lib.GROW_CONTINUOUS, _lib.SPLIT_SCALE]
