"""``densify.swap_rows_``: the one optimizer surgery behind ``densify_and_prune`` (both paths), ``mcmc.add_new_gs`` and
``layout``'s row moves.  The same assertions run on a direct call and through ``layout.reorder_gaussians_``.  CPU only."""
import torch
from torch import nn

from mvs_gaussian_splatting_amd.densify import GROUP_ATTR, swap_rows_
from mvs_gaussian_splatting_amd.layout import reorder_gaussians_

P = 5
SHAPES = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, 15, 3), "opacity": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
STEPPED = ("xyz", "f_dc")      # groups that hold Adam's state after the one step
NO_STATE = "f_rest"            # a group that has not stepped yet
ODD_STATE = "scaling"          # a group whose state dict has no moments
UNOWNED = ("opacity", "rotation")      # no group: a plain tensor that wants gradients, and a frozen Parameter


class _Model:
    pass


def _model():
    g = torch.Generator().manual_seed(11)
    m = _Model()
    for k, a in GROUP_ATTR.items():
        setattr(m, a, nn.Parameter(torch.randn(*SHAPES[k], generator=g)))
    m._opacity = m._opacity.detach().clone().requires_grad_(True)
    m._rotation = nn.Parameter(m._rotation.detach().clone(), requires_grad=False)
    m.optimizer = torch.optim.Adam([{"params": [getattr(m, GROUP_ATTR[k])], "lr": 1e-2, "name": k}
                                    for k in GROUP_ATTR if k not in UNOWNED], lr=0.0, eps=1e-15)
    for k in STEPPED:
        getattr(m, GROUP_ATTR[k]).grad = torch.randn(*SHAPES[k], generator=g)
    m.optimizer.step()
    m.optimizer.state[m._scaling] = {"step": torch.tensor(3.0), "note": "kept"}
    return m


def _snapshot(m):
    state = {k: dict(m.optimizer.state[getattr(m, GROUP_ATTR[k])]) for k in STEPPED + (ODD_STATE,)}
    assert all(set(state[k]) >= {"step", "exp_avg", "exp_avg_sq"} for k in STEPPED)
    assert len(m.optimizer.state) == len(state)
    return {k: getattr(m, a).detach().clone() for k, a in GROUP_ATTR.items()}, state


def _assert_swapped(m, params, state, index):
    groups = {grp["name"]: grp["params"][0] for grp in m.optimizer.param_groups}
    for k, a in GROUP_ATTR.items():
        t = getattr(m, a)
        assert torch.equal(t.detach(), params[k][index])
        if k in UNOWNED:
            continue
        assert t is groups[k] and isinstance(t, nn.Parameter) and t.requires_grad
    # no entry is left under a dead parameter: the state's keys are the parameters of the groups that had state
    assert len(m.optimizer.state) == len(state)
    assert all(any(p is q for q in groups.values()) for p in m.optimizer.state)
    for k in STEPPED:
        now = m.optimizer.state[groups[k]]
        assert set(now) == set(state[k])
        assert now["step"] is state[k]["step"]                             # carried over as it is
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(now[key], state[k][key][index])
    assert groups[NO_STATE] not in m.optimizer.state
    odd = m.optimizer.state[groups[ODD_STATE]]                             # moved, not stranded
    assert set(odd) == {"step", "note"} and odd["step"] is state[ODD_STATE]["step"] and odd["note"] == "kept"
    assert not isinstance(m._opacity, nn.Parameter) and m._opacity.requires_grad
    assert isinstance(m._rotation, nn.Parameter) and not m._rotation.requires_grad
    # the optimizer goes on from the moved state
    for k in STEPPED:
        groups[k].grad = torch.ones_like(groups[k])
    m.optimizer.step()
    assert all(float(m.optimizer.state[groups[k]]["step"]) == 2.0 for k in STEPPED)


def test_swap_rows_moves_parameters_state_and_moments():
    m = _model()
    params, state = _snapshot(m)
    index = torch.tensor([4, 0, 0, 2])                                     # the row count changes
    seen = []

    def moment(t):
        seen.append(t)
        return t[index].contiguous()
    swap_rows_(m, GROUP_ATTR, {k: v[index].contiguous() for k, v in params.items()}, moment)
    # both moments of every stepped group went through the callable, and nothing else did
    assert len(seen) == 2 * len(STEPPED)
    assert all(any(t is state[k][key] for t in seen) for k in STEPPED for key in ("exp_avg", "exp_avg_sq"))
    _assert_swapped(m, params, state, index)


def test_reorder_gaussians_goes_through_the_same_swap():
    m = _model()
    params, state = _snapshot(m)
    perm = torch.tensor([3, 1, 4, 0, 2])
    reorder_gaussians_(m, perm)
    _assert_swapped(m, params, state, perm)


def test_swap_rows_without_an_optimizer_keeps_the_kinds():
    m = _model()
    params, _ = _snapshot(m)
    del m.optimizer
    index = torch.tensor([1, 3])
    swap_rows_(m, GROUP_ATTR, {k: v[index].contiguous() for k, v in params.items()}, lambda t: t[index])
    for k, a in GROUP_ATTR.items():
        assert torch.equal(getattr(m, a).detach(), params[k][index])
    assert isinstance(m._xyz, nn.Parameter) and m._xyz.requires_grad
    assert not isinstance(m._opacity, nn.Parameter) and m._opacity.requires_grad
    assert isinstance(m._rotation, nn.Parameter) and not m._rotation.requires_grad
