"""CPU-side checks of the joint-frame reference (tests/joint_restate.py) that tests/test_gpu_joint_frame.py compares the HIP
path with: the conditions it is built under hold on the oracle alone, and the bars the GPU test sets -- grad_util.compare_grads,
max(1e-5, 2 x the float32 restatement's own error), never above ESCAPE_CAP -- are reachable in float32.  Run with -s for the
left-out shares, the five coefficients and the float32-versus-float64 errors per tensor."""
import pytest
import torch

from grad_util import ESCAPE_CAP, compare_grads
from joint_restate import MAX_LEFT_OUT, N_USER, TERMS, bar_of, joint_reference, leaf_names, present
from median_restate import SCENES, reference

CASES = [("small", False), ("big", False), ("small", True)]
IDS = ["small", "big", "small-cov3D"]


@pytest.mark.parametrize("name,use_cov", CASES, ids=IDS)
def test_the_caps_hold_on_the_oracle_alone_and_the_bars_are_reachable_in_float32(name, use_cov):
    ref = joint_reference(name, use_cov)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    label = name + (", cov3D_precomp" if use_cov else "")
    print(f"[joint host] {label}: left out " + ", ".join(f"{t} {ref['left_out'][t]:.4f} (cap {MAX_LEFT_OUT[t]})"
                                                          for t in TERMS))
    print(f"[joint host] {label}: coefficients " + ", ".join(f"{t} {ref['coef'][t]:.6e}" for t in TERMS))
    for t in TERMS:
        assert 0.0 <= ref["left_out"][t] <= MAX_LEFT_OUT[t], t
        assert float(ref["weights"][t].abs().max()) > 0.0
    assert ref["names"] == leaf_names(use_cov)
    # every term's coefficient-weighted position gradient has max-norm one: none hides under another in the sum
    for t in TERMS:
        top = ref["coef"][t] * float(r64["terms"][t]["xyz"].abs().max())
        assert abs(top - 1.0) <= 1e-12, (t, top)
    # the joint float32 sum against the joint float64 sum: the GPU test's bar, met by an independent float32 evaluation
    for k in ref["names"]:
        bar, e32 = bar_of(r64["joint"][k], r32["joint"][k])
        print(f"[joint host] {label}: joint {k}: float32 restatement {e32:.2e}, bar {bar:.2e} (cap {ESCAPE_CAP:.0e})")
        assert e32 <= bar <= ESCAPE_CAP, k
    compare_grads(r32["joint"], r64["joint"], r32["joint"], f"joint frame, {label}, float32 restatement")
    # ... and term by term (the bars of the additivity test)
    for t in TERMS:
        compare_grads(present(r32["terms"][t]), present(r64["terms"][t]), present(r32["terms"][t]),
                      f"joint frame, {label}, {t} alone, float32 restatement")
    # the densification statistic the trainer reads on such a frame: ||d joint / d means2D[:, :2]||
    want, want32 = (r["joint"]["means2D"][:, :2].norm(dim=1).double() for r in (r64, r32))
    e32 = float((want32 - want).abs().max()) / float(want.abs().max())
    print(f"[joint host] {label}: norm of the joint means2D gradient: float32 restatement {e32:.2e}")
    assert max(1e-5, 2.0 * e32) <= ESCAPE_CAP


@pytest.mark.parametrize("name,use_cov", CASES, ids=IDS)
def test_each_term_depends_on_what_its_node_differentiates(name, use_cov):
    ref = joint_reference(name, use_cov)
    geometry = set(ref["names"]) - {"f_dc", "f_rest", "F"}
    depends = {"colour": geometry | {"f_dc", "f_rest"}, "aux": geometry, "features": geometry | {"F"},
               "distortion": geometry, "median": {"xyz"}}
    for dt in (torch.float64, torch.float32):
        for t in TERMS:
            for k in ref["names"]:
                g = ref[dt]["terms"][t][k]
                if k in depends[t]:
                    assert g is not None and g.dtype == dt and float(g.abs().max()) > 0.0, (t, k)
                else:
                    assert g is None, f"the {t} term has a gradient for {k}"
        assert float(ref[dt]["joint"]["means2D"][:, 2].abs().max()) == 0.0
    assert tuple(ref["F"].shape) == (SCENES[name]["P"], N_USER) and ref["F"].dtype == torch.float32
    assert tuple(ref["maps"]["features"].shape) == (N_USER + 3, SCENES[name]["height"], SCENES[name]["width"])


def test_the_joint_reference_is_the_single_term_references_on_the_same_frame():
    """The median term of the joint reference is tests/median_restate.reference (same scene, same weights): one oracle
    pass feeds all five terms without changing any of them."""
    ref, alone = joint_reference("small"), reference("small")
    assert torch.equal(ref["weights"]["median"], alone["weights"])
    assert torch.equal(ref["maps"]["median"], alone[torch.float64]["median"])
    assert torch.equal(ref["maps"]["median_id"], alone[torch.float64]["id"])
    for dt in (torch.float64, torch.float32):
        assert torch.equal(ref[dt]["terms"]["median"]["xyz"], alone[dt]["grads"]["xyz"])
    assert torch.equal(ref["radii"], alone["radii"])


def test_the_big_scene_exercises_more_than_one_round():
    aux = joint_reference("big")["aux"]
    assert int((aux["ranges"][:, 1] - aux["ranges"][:, 0]).max()) > 256, "a list must exceed one 256-entry round"
    assert int(aux["n_contrib"].max()) > 256, "a pixel must composite past the first round"
    assert int(aux["pre"]["tiles_touched"].max()) > 64, "a Gaussian must have more than 64 instances"
