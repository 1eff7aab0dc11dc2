"""The fork's densify_and_prune on CPU: the float32 restatement (tests/densify_fork_restate.py) against the reference
class's own results (tests/golden/densify_fork.npz, make_golden_densify_fork.py) -- counts, row order, values and
Adam moments, bit for bit -- plus the branch predicate, the draw-shape rules and the host-side input checks of
mvs_gaussian_splatting_amd.densify."""
import os
import types

import numpy as np
import pytest
import torch

from densify_fork_restate import FLAG_NAMES, densify_and_prune, split_draw_rows
from mvs_gaussian_splatting_amd import densify

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "densify_fork.npz")
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "dirs_prob", "conti_dirs", "grow_dist",
          "split_distance", "split_scale")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIXTURE)


def cases(fx):
    return sorted({k.split("/")[0] for k in fx.files})


def load_case(fx, case):
    flags = dict(zip(FLAG_NAMES, (bool(v) for v in fx[f"{case}/flags"])))
    args = fx[f"{case}/args"]
    names = [k for k in GROUPS if f"{case}/in/param/{k}" in fx.files]
    params = {k: torch.from_numpy(fx[f"{case}/in/param/{k}"]) for k in names}
    moments = {k: (torch.from_numpy(fx[f"{case}/in/exp_avg/{k}"]), torch.from_numpy(fx[f"{case}/in/exp_avg_sq/{k}"]))
               for k in names}
    dirs = torch.from_numpy(fx[f"{case}/dirs"]) if f"{case}/dirs" in fx.files else None
    return dict(flags=flags, names=names, params=params, moments=moments, dirs=dirs,
                accum=torch.from_numpy(fx[f"{case}/in/xyz_gradient_accum"]),
                denom=torch.from_numpy(fx[f"{case}/in/denom"]),
                noise=torch.from_numpy(fx[f"{case}/noise"]), dir_noise=torch.from_numpy(fx[f"{case}/dir_noise"]),
                max_grad=float(args[0]), min_opacity=float(args[1]), extent=float(args[2]),
                max_screen_size=None if args[3] < 0 else float(args[3]), percent_dense=float(args[4]),
                iteration=int(args[5]), reset=int(args[6]))


def restate(c):
    return densify_and_prune(c["params"], c["moments"], c["accum"], c["denom"], c["flags"], c["percent_dense"],
                             c["max_grad"], c["min_opacity"], c["extent"], c["max_screen_size"], c["iteration"],
                             c["reset"], dirs=c["dirs"], noise=c["noise"], dir_noise=c["dir_noise"])


def test_fixture_covers_the_issue_cases(fx):
    cs = cases(fx)
    assert len(cs) >= 11
    flags = {c: dict(zip(FLAG_NAMES, fx[f"{c}/flags"])) for c in cs}
    grow = {c for c in cs if fx[f"{c}/args"][5] > fx[f"{c}/args"][6] and (flags[c]["grow_dir"] or flags[c]["continous_dir"])}
    assert any(flags[c]["prob_notreinit"] for c in grow) and any(flags[c]["continous_dir"] for c in grow)
    assert any(flags[c]["symmetric_split"] for c in grow) and any(flags[c]["learn_split_distance"] for c in grow)
    assert any(flags[c]["split_notreinit"] for c in cs if c not in grow)
    assert any(fx[f"{c}/out/param/xyz"].shape[0] == 0 for c in cs)                         # everything pruned
    assert any(fx[f"{c}/in/param/dirs_prob"].shape[1] == 128 for c in cs if f"{c}/in/param/dirs_prob" in fx.files)


@pytest.mark.parametrize("case", sorted({k.split("/")[0] for k in np.load(FIXTURE).files}))
def test_restatement_matches_reference(fx, case):
    c = load_case(fx, case)
    params, moments, info = restate(c)
    n_out = fx[f"{case}/out/param/xyz"].shape[0]
    assert set(params) == set(c["names"])
    for k in c["names"]:
        assert torch.equal(params[k], torch.from_numpy(fx[f"{case}/out/param/{k}"])), (case, k)
        assert torch.equal(moments[k][0], torch.from_numpy(fx[f"{case}/out/exp_avg/{k}"])), (case, k, "exp_avg")
        assert torch.equal(moments[k][1], torch.from_numpy(fx[f"{case}/out/exp_avg_sq/{k}"])), (case, k, "exp_avg_sq")
        assert params[k].shape[0] == n_out
    # the draws the reference consumed: split rows of its order, one continuous re-init draw per selected Gaussian
    assert c["noise"].shape[0] == split_draw_rows(c["flags"], info["split_rows"])
    conti_reinit = info["branch"] == "grow" and c["flags"]["continous_dir"] and not c["flags"]["prob_notreinit"]
    assert c["dir_noise"].shape[0] == (info["selected"] if conti_reinit else 0)


def test_branch_predicate():
    opt = types.SimpleNamespace(opacity_reset_interval=3000)
    plain = types.SimpleNamespace()
    assert densify.branch(plain) == densify.CLONE_SPLIT
    assert densify.branch(types.SimpleNamespace(learn_split_distance=True)) == densify.CLONE_SPLIT
    for flag in ("grow_dir", "continous_dir"):
        m = types.SimpleNamespace(**{flag: True})
        assert densify.branch(m, opt, 3000) == densify.CLONE_SPLIT        # `iteration > opacity_reset_interval`
        assert densify.branch(m, opt, 3001) == densify.GROW
        assert densify.branch(m, opt, 100) == densify.CLONE_SPLIT
        with pytest.raises(ValueError, match="opt and iteration"):
            densify.branch(m)
        with pytest.raises(ValueError, match="opt and iteration"):
            densify.branch(m, opt, None)
    m = types.SimpleNamespace(grow_distance=True)                          # no direction flag: never grows
    assert densify.branch(m, opt, 5000) == densify.CLONE_SPLIT


def test_draw_rows_rule():
    f = dict.fromkeys(FLAG_NAMES, False)
    assert split_draw_rows(f, 7) == 14
    assert split_draw_rows(dict(f, symmetric_split=True), 7) == 7
    assert split_draw_rows(dict(f, learn_split_distance=True, symmetric_split=True), 7) == 0


def _model(P=5, **flags):
    m = types.SimpleNamespace(_xyz=torch.zeros(P, 3), num_dirs=4, dirs=torch.zeros(4, 3), **flags)
    m.modelcg = types.SimpleNamespace()
    return m


def test_fork_detection_and_input_checks():
    assert not densify.is_fork(_model())
    assert densify.is_fork(_model(grow_distance=True))
    m = _model(grow_dir=True)
    with pytest.raises(ValueError, match="no _dirs_prob"):
        densify._fork_inputs(m, 5)
    m._dirs_prob = torch.zeros(5, 3)
    with pytest.raises(ValueError, match=r"_dirs_prob: expected float32 \[5, 4\]"):
        densify._fork_inputs(m, 5)
    m._dirs_prob = torch.zeros(5, 4)
    flags, learned = densify._fork_inputs(m, 5)
    assert list(learned) == ["dirs_prob"] and flags["grow_dir"] and not flags["prob_notreinit"]
    m.learn_split_scale = True
    m._split_scale = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="_split_scale"):
        densify._fork_inputs(m, 5)
    m = _model(grow_distance=True, _split_distance=torch.zeros(5, 3), _grow_dist=torch.zeros(5, 1))
    assert densify.is_fork(m)
    with pytest.raises(ValueError, match="learn_split_distance is off"):
        densify._fork_inputs(m, 5)
    with pytest.raises(ValueError, match="exclusive"):
        densify._fork_inputs(_model(grow_dir=True, continous_dir=True), 5)
    m = _model(grow_dir=True, _dirs_prob=torch.zeros(5, 4))
    m.num_dirs = 0
    with pytest.raises(ValueError, match="num_dirs"):
        densify._fork_inputs(m, 5)
