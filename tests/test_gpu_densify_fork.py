"""The fork's densify_and_prune on the HIP path (csrc/densify_fork.hip, mvs_gaussian_splatting_amd/densify.py):
against the reference class's results (tests/golden/densify_fork.npz) in every recorded case, against the float32
restatement at a few thousand Gaussians, with spatial_order, and inside a fork training loop with the render gate
open across opacity_reset_interval.

Copies, Adam moments and re-init constants are bit-identical; the computed rows (grown xyz, the children's xyz and
scaling, the normalised conti_dirs re-init) agree to 1e-6 relative (exp / log / sigmoid / sqrt and a 3x3 product in
float32, as tests/test_gpu_densify.py allows)."""
import types

import numpy as np
import pytest
import torch
from torch import nn

from conftest import small_scene
from densify_fork_restate import FLAG_NAMES, densify_and_prune as restate
from test_densify_fork_host import FIXTURE, GROUPS, load_case

pytestmark = pytest.mark.gpu
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
        "scaling": "_scaling", "rotation": "_rotation", "dirs_prob": "_dirs_prob", "conti_dirs": "_conti_dirs",
        "grow_dist": "_grow_dist", "split_distance": "_split_distance", "split_scale": "_split_scale"}
COMPUTED = ("xyz", "scaling", "conti_dirs")
CASES = sorted({k.split("/")[0] for k in np.load(FIXTURE).files})


class ForkModel:
    """The attributes of the fork's GaussianModel that densification reads, with a torch.optim.Adam over named
    groups (training_setup, scene/gaussian_model.py:240-266)."""

    def __init__(self, params, moments, flags, accum, denom, dirs, dev, percent_dense=0.01):
        self.percent_dense = percent_dense
        for f in ("grow_dir", "continous_dir", "grow_distance", "learn_split_distance", "learn_split_scale"):
            setattr(self, f, bool(flags[f]))
        self.modelcg = types.SimpleNamespace(**{f: bool(flags[f]) for f in FLAG_NAMES})
        self.num_dirs = int(dirs.shape[0]) if dirs is not None else 128
        if dirs is not None:
            self.dirs = dirs.to(dev)
        for k, t in params.items():
            setattr(self, ATTR[k], nn.Parameter(t.detach().clone().to(dev).requires_grad_(True)))
        self.optimizer = torch.optim.Adam([{"params": [getattr(self, ATTR[k])], "lr": 1e-3, "name": k}
                                           for k in params], lr=0.0, eps=1e-15)
        if moments is not None:
            for k in params:
                self.optimizer.state[getattr(self, ATTR[k])] = {
                    "step": torch.tensor(1.0), "exp_avg": moments[k][0].clone().to(dev),
                    "exp_avg_sq": moments[k][1].clone().to(dev)}
        self.xyz_gradient_accum = accum.clone().to(dev)
        self.denom = denom.clone().to(dev)
        self.max_radii2D = torch.zeros(accum.shape[0], device=dev)

    def tensors(self, names):
        out = {}
        for k in names:
            p = getattr(self, ATTR[k])
            st = self.optimizer.state[p]
            out[k] = (p.detach().cpu(), st["exp_avg"].cpu(), st["exp_avg_sq"].cpu())
        return out


def _hip(c, dev, spatial_order=False):
    from mvs_gaussian_splatting_amd.densify import densify_and_prune
    m = ForkModel(c["params"], c["moments"], c["flags"], c["accum"], c["denom"], c["dirs"], dev, c["percent_dense"])
    info = densify_and_prune(m, c["max_grad"], c["min_opacity"], c["extent"], c["max_screen_size"],
                             noise=c["noise"].to(dev), spatial_order=spatial_order,
                             opt=types.SimpleNamespace(opacity_reset_interval=c["reset"]), iteration=c["iteration"],
                             dir_noise=c["dir_noise"].to(dev))
    return m, info


def _close(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = ((got - want).abs() / want.abs().clamp(min=1.0)).max() if got.numel() else torch.tensor(0.0)
    assert float(err) <= 1e-6, (what, float(err))


def _compare(m, names, want, what):
    got = m.tensors(names)
    n = int(want["xyz"][0].shape[0])
    assert m.xyz_gradient_accum.shape == (n, 1) and m.denom.shape == (n, 1) and m.max_radii2D.shape == (n,)
    assert not (m.xyz_gradient_accum.any() or m.denom.any() or m.max_radii2D.any())
    for k in names:
        (gp, ga, gb), (wp, wa, wb) = got[k], want[k]
        if k in COMPUTED:
            _close(gp, wp, f"{what}/{k}")
        else:
            assert torch.equal(gp, wp), f"{what}/{k}"
        assert torch.equal(ga, wa), f"{what}/{k}/exp_avg"
        assert torch.equal(gb, wb), f"{what}/{k}/exp_avg_sq"


@pytest.mark.parametrize("case", CASES)
def test_hip_matches_the_reference(gpu_device, case):
    fx = np.load(FIXTURE)
    c = load_case(fx, case)
    m, info = _hip(c, gpu_device)
    want = {k: tuple(torch.from_numpy(fx[f"{case}/out/{t}/{k}"]) for t in ("param", "exp_avg", "exp_avg_sq"))
            for k in c["names"]}
    assert info["points"] == want["xyz"][0].shape[0]
    assert info["branch"] == ("grow" if case.startswith("grow") else "clone_split")
    _compare(m, c["names"], want, case)
    # the optimizer survives the surgery: one Adam step over every group
    for grp in m.optimizer.param_groups:
        grp["params"][0].grad = torch.ones_like(grp["params"][0])
    m.optimizer.step()


def _random_case(P, seed, flags, nd=128, iteration=3100):
    g = torch.Generator().manual_seed(seed)
    params = {"xyz": torch.randn(P, 3, generator=g) * 2.0, "f_dc": torch.randn(P, 1, 3, generator=g),
              "f_rest": 0.1 * torch.randn(P, 15, 3, generator=g),
              "opacity": 2.5 * torch.randn(P, 1, generator=g) - 1.0,
              "scaling": float(np.log(0.05)) + 1.2 * torch.randn(P, 3, generator=g),
              "rotation": torch.randn(P, 4, generator=g)}
    widths = {"dirs_prob": nd, "conti_dirs": 3, "grow_dist": 1, "split_distance": 3, "split_scale": 1}
    for k, f in (("dirs_prob", "grow_dir"), ("conti_dirs", "continous_dir"), ("grow_dist", "grow_distance"),
                 ("split_distance", "learn_split_distance"), ("split_scale", "learn_split_scale")):
        if flags.get(f):
            params[k] = torch.randn(P, widths[k], generator=g)
    moments = {k: (torch.randn(t.shape, generator=g), torch.rand(t.shape, generator=g)) for k, t in params.items()}
    denom = torch.randint(0, 4, (P, 1), generator=g).float()
    accum = torch.rand(P, 1, generator=g) * 0.0006 * denom
    th = np.pi * (3 - np.sqrt(5)) * np.arange(nd)
    zz = np.linspace(1 - 1.0 / nd, 1.0 / nd - 1, nd)
    r = np.sqrt(1 - zz * zz)
    dirs = torch.tensor(np.stack([r * np.cos(th), r * np.sin(th), zz], 1), dtype=torch.float32) if flags.get(
        "grow_dir") else None
    full = {f: bool(flags.get(f, False)) for f in FLAG_NAMES}
    c = dict(flags=full, names=list(params), params=params, moments=moments, dirs=dirs, accum=accum, denom=denom,
             max_grad=0.0002, min_opacity=0.005, extent=5.0, max_screen_size=20.0, percent_dense=0.01,
             iteration=iteration, reset=3000)
    # the draws: count the split rows and the selected Gaussians from the restatement's own selection
    _, _, info = restate(params, moments, accum, denom, full, 0.01, 0.0002, 0.005, 5.0, 20.0, iteration, 3000,
                         dirs=dirs, noise=torch.zeros(4 * P, 3), dir_noise=torch.zeros(P, 3))
    from densify_fork_restate import split_draw_rows
    c["noise"] = torch.randn(split_draw_rows(full, info["split_rows"]), 3, generator=g)
    conti = info["branch"] == "grow" and full["continous_dir"] and not full["prob_notreinit"]
    c["dir_noise"] = torch.randn(info["selected"] if conti else 0, 3, generator=g)
    return c


RANDOM = {
    "grow_dir128_learned": dict(grow_dir=True, grow_distance=True, learn_split_distance=True, learn_split_scale=True),
    "grow_conti_symmetric": dict(continous_dir=True, grow_distance=True, symmetric_split=True),
    "clone_split_dirs": dict(grow_dir=True, learn_split_scale=True, split_notreinit=True),
}


@pytest.mark.parametrize("name", list(RANDOM))
def test_hip_matches_the_restatement_at_4k(gpu_device, name):
    _matches_the_restatement(gpu_device, name, 4096)


@pytest.mark.parametrize("P", [256 * 32 + 1, 256 * 33 + 1])
@pytest.mark.parametrize("name", list(RANDOM))
def test_hip_matches_the_restatement_past_one_scan_line(gpu_device, name, P):
    """33 and 34 blocks of 256 rows: the block-counter scan moves a whole 32-entry line, and nb + 1 is no multiple of 4."""
    _matches_the_restatement(gpu_device, name, P)


def _matches_the_restatement(gpu_device, name, P):
    c = _random_case(P, 7 + len(name), RANDOM[name], iteration=1000 if name.startswith("clone") else 3100)
    p, mo, info = restate(c["params"], c["moments"], c["accum"], c["denom"], c["flags"], 0.01, c["max_grad"],
                          c["min_opacity"], c["extent"], c["max_screen_size"], c["iteration"], c["reset"],
                          dirs=c["dirs"], noise=c["noise"], dir_noise=c["dir_noise"])
    m, hinfo = _hip(c, gpu_device)
    assert hinfo["selected"] == info["selected"] and hinfo["branch"] == info["branch"]
    assert hinfo["points"] == p["xyz"].shape[0] > P
    _compare(m, c["names"], {k: (p[k], mo[k][0], mo[k][1]) for k in c["names"]}, name)


def test_spatial_order_is_the_reference_order_permuted(gpu_device):
    from mvs_gaussian_splatting_amd.layout import morton_permutation
    c = _random_case(3000, 3, RANDOM["grow_dir128_learned"])
    a, _ = _hip(c, gpu_device)
    b, info = _hip(c, gpu_device, spatial_order=True)
    perm = morton_permutation(a._xyz.detach()).cpu()
    ta, tb = a.tensors(c["names"]), b.tensors(c["names"])
    for k in c["names"]:
        for j in range(3):
            assert torch.equal(ta[k][j][perm], tb[k][j]), k
    assert b._dirs_prob.shape[0] == info["points"]


def test_plain_models_keep_the_plain_path(gpu_device):
    """A model without fork flags or tensors returns the plain dict: no 'branch' key, no 'selected'."""
    from mvs_gaussian_splatting_amd.densify import densify_and_prune
    c = _random_case(1000, 5, {})
    m = ForkModel(c["params"], c["moments"], c["flags"], c["accum"], c["denom"], None, gpu_device)
    for f in ("grow_dir", "continous_dir", "grow_distance", "learn_split_distance", "learn_split_scale"):
        delattr(m, f)
    info = densify_and_prune(m, 0.0002, 0.005, 5.0, 20)
    assert set(info) == {"points", "kept", "cloned", "split_selected", "children_per_copy"}


def test_draw_and_flag_errors(gpu_device):
    from mvs_gaussian_splatting_amd.densify import densify_and_prune
    c = _random_case(500, 9, RANDOM["grow_conti_symmetric"])
    opt = types.SimpleNamespace(opacity_reset_interval=3000)
    m = ForkModel(c["params"], c["moments"], c["flags"], c["accum"], c["denom"], None, gpu_device)
    with pytest.raises(ValueError, match="noise must be"):
        densify_and_prune(m, 0.0002, 0.005, 5.0, 20, noise=torch.zeros(3, 3, device=gpu_device), opt=opt,
                          iteration=3100)
    with pytest.raises(ValueError, match="dir_noise must be"):
        densify_and_prune(m, 0.0002, 0.005, 5.0, 20, noise=c["noise"].to(gpu_device), opt=opt, iteration=3100,
                          dir_noise=torch.zeros(1, 3, device=gpu_device))
    with pytest.raises(ValueError, match="opt and iteration"):
        densify_and_prune(m, 0.0002, 0.005, 5.0, 20)
    m._grow_dist = None
    with pytest.raises(ValueError, match="no _grow_dist"):
        densify_and_prune(m, 0.0002, 0.005, 5.0, 20, opt=opt, iteration=3100)


def test_fork_training_loop_with_the_gate_open(gpu_device):
    """train.py:91/:134 on the HIP path: render with the grow gate open, loss, backward, densification statistics, the
    fork's densification every few steps across opacity_reset_interval, then the optimizer step."""
    from mvs_gaussian_splatting_amd import add_densification_stats, render
    from mvs_gaussian_splatting_amd.densify import densify_and_prune
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    opt_args = types.SimpleNamespace(densify_from_iter=500, densification_interval=100, densify_until_iter=15000,
                                     opacity_reset_interval=3000)
    model, cam, bg, target = small_scene(P=3000, sh_degree=3, scale=0.05, seed=1)
    P = model._xyz.shape[0]
    g = torch.Generator().manual_seed(11)
    nd = 32
    th = np.pi * (3 - np.sqrt(5)) * np.arange(nd)
    zz = np.linspace(1 - 1.0 / nd, 1.0 / nd - 1, nd)
    r = np.sqrt(1 - zz * zz)
    model.to(gpu_device)
    cam.to(gpu_device)
    bg, target = bg.to(gpu_device), target.to(gpu_device)
    fork = model                          # the synthetic model's getters, with the fork's attributes added
    fork.percent_dense, fork.num_dirs = 0.01, nd
    fork.grow_dir, fork.continous_dir, fork.grow_distance = True, False, True
    fork.learn_split_distance = fork.learn_split_scale = False
    fork.modelcg = types.SimpleNamespace(learn_split_distance=False, learn_split_scale=False, symmetric_split=False,
                                         split_notreinit=False, prob_notreinit=False)
    fork.dirs = torch.tensor(np.stack([r * np.cos(th), r * np.sin(th), zz], 1), dtype=torch.float32,
                             device=gpu_device)
    for k in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"):
        setattr(fork, ATTR[k], nn.Parameter(getattr(model, ATTR[k]).detach().clone()))
    fork._dirs_prob = nn.Parameter(torch.randn(P, nd, generator=g).to(gpu_device))
    fork._grow_dist = nn.Parameter(torch.randn(P, 1, generator=g).to(gpu_device))
    names = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "dirs_prob", "grow_dist")
    fork.optimizer = torch.optim.Adam([{"params": [getattr(fork, ATTR[k])], "lr": 1e-3, "name": k} for k in names],
                                      lr=0.0, eps=1e-15)
    for a in ("xyz_gradient_accum", "denom"):
        setattr(fork, a, torch.zeros(P, 1, device=gpu_device))
    fork.max_radii2D = torch.zeros(P, device=gpu_device)
    pipe = PipelineParams()
    counts, branches, thr = [], [], 2e-6
    for it in range(2980, 3030):
        pkg = render(cam, fork, pipe, bg, grow_dir=True, grow_distance=True, iteration=it,
                     densify_grad_threshold=thr, opt=opt_args, cameras_extent=2.0, modelcg=fork.modelcg)
        loss = (pkg["render"] - target).abs().mean()
        assert torch.isfinite(loss), it
        loss.backward()
        add_densification_stats(fork, pkg["viewspace_points"], pkg["radii"])
        fork.optimizer.step()
        fork.optimizer.zero_grad(set_to_none=True)
        if it % 5 == 4:
            grad = (fork.xyz_gradient_accum / fork.denom).nan_to_num(0.0)
            if bool((grad > 0).any()):                 # densify the top fifth of the Gaussians that were seen
                thr = float(torch.quantile(grad[grad > 0], 0.8))
            info = densify_and_prune(fork, thr, 0.005, 2.0, 20, opt=opt_args, iteration=it)
            branches.append(info["branch"])
            n = fork._xyz.shape[0]
            counts.append((n, info["selected"]))
            for k in names:
                p = getattr(fork, ATTR[k])
                assert p.shape[0] == n, (it, k)
                st = fork.optimizer.state.get(p, {})       # Adam creates a group's state at its first gradient
                assert all(st[m].shape[0] == n for m in ("exp_avg", "exp_avg_sq") if m in st), (it, k)
            assert fork.xyz_gradient_accum.shape[0] == n and fork.max_radii2D.shape[0] == n
    assert "grow" in branches and "clone_split" in branches, branches
    assert all("exp_avg" in fork.optimizer.state[getattr(fork, ATTR[k])] for k in names)
    assert any(s > 0 for _, s in counts) and counts[-1][0] != P, counts
