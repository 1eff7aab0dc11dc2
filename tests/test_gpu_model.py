"""GaussianModel on the MI355X (mvs_gaussian_splatting_amd/model.py, trainer.py, csrc/model.hip) against the
reference's own results (tests/golden/model_lifecycle.npz): create_from_pcd, reset_opacity and the optimizer step behind
it, the opacity sparsity term and its gradient, both without a host round-trip (checked by capturing them into a HIP
graph: a synchronising call fails the capture), and the training loop of examples/train.py: checkpoint + resume is
bit-identical to the uninterrupted run, the loss falls, the PLY round-trips.

Bars: copies bit-exact; computed rows |got - want| / max(|want|, 1) <= 1e-6 (the densify tests' bar); the sparsity
value 1e-6 relative to the float64 value; its gradient max|got - want| <= 1e-5 max|want| and exactly zero off the set."""
import os
import sys
import types

import numpy as np
import pytest
import torch
from torch import nn

from test_model_host import FIXTURE, GROUP_ATTR, ROOT, fixture_opt

pytestmark = pytest.mark.gpu
FORK_ATTR = {"dirs_prob": "_dirs_prob", "conti_dirs": "_conti_dirs", "grow_dist": "_grow_dist",
             "split_distance": "_split_distance", "split_scale": "_split_scale"}
PCD_CASES = {"plain": dict(), "grow_dir": dict(grow_dir=True, num_dirs=128), "continous_dir": dict(continous_dir=True),
             "dist_splits": dict(grow_distance=True, modelcg=types.SimpleNamespace(learn_split_distance=True,
                                                                                   learn_split_scale=True))}
COMPUTED = ("f_dc", "scaling", "opacity", "conti_dirs")


def _close(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = ((got - want).abs() / want.abs().clamp(min=1.0)).max() if got.numel() else torch.tensor(0.0)
    print(f"{what}: max error {float(err):.3e} (bar 1e-6)")
    assert float(err) <= 1e-6, (what, float(err))


def _optimizer_cls(name):
    from mvs_gaussian_splatting_amd import optim
    return torch.optim.Adam if name == "torch" else optim.Adam


def _example():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train as example
    return example


# ---- 5. create_from_pcd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(PCD_CASES))
def test_create_from_pcd_matches_the_reference(gpu_device, case):
    from mvs_gaussian_splatting_amd import GaussianModel
    fx = np.load(FIXTURE)
    m = GaussianModel(int(fx[f"pcd/{case}/sh_degree"]), **PCD_CASES[case])
    noise = torch.from_numpy(fx[f"pcd/{case}/dir_noise"]) if case == "continous_dir" else None
    m.create_from_pcd(fx["pcd/points"], fx["pcd/colors"], float(fx["pcd/spatial_lr_scale"]), dir_noise=noise,
                      dist2=torch.from_numpy(fx["pcd/dist2"]), device=gpu_device)
    assert m.spatial_lr_scale == float(fx["pcd/spatial_lr_scale"]) and m.active_sh_degree == 0
    seen = 0
    for k, a in {**GROUP_ATTR, **FORK_ATTR}.items():
        key = f"pcd/{case}/{k}"
        if key not in fx.files:
            assert not hasattr(m, a) or getattr(m, a).numel() == 0, (case, a)
            continue
        got, want = getattr(m, a), torch.from_numpy(fx[key])
        assert isinstance(got, nn.Parameter) and got.requires_grad and got.is_cuda and got.is_contiguous(), (case, a)
        if k in COMPUTED:
            _close(got.detach().cpu(), want, f"{case}/{k}")
        else:
            assert torch.equal(got.detach().cpu(), want), (case, k)
        seen += 1
    assert seen >= 6
    assert torch.equal(m.max_radii2D.cpu(), torch.from_numpy(fx[f"pcd/{case}/max_radii2D"]))
    if case == "grow_dir":
        assert m.dirs.is_cuda and torch.equal(m.dirs.cpu(), torch.from_numpy(fx["pcd/grow_dir/dirs"]))
    clamped = fx["pcd/dist2"] < 1e-7                                 # the clamp of :210 was exercised
    assert clamped.sum() == 3 and torch.isfinite(m._scaling).all()


def test_create_from_pcd_with_the_real_knn(gpu_device):
    from mvs_gaussian_splatting_amd import GaussianModel
    fx = np.load(FIXTURE)
    m = GaussianModel(3).create_from_pcd(types.SimpleNamespace(points=fx["pcd/points"], colors=fx["pcd/colors"]), 2.0,
                                         device=gpu_device)
    assert m.spatial_lr_scale == 2.0
    d2 = torch.from_numpy(fx["pcd/dist2_exact"]).clamp_min(1e-7)     # scipy.spatial.cKDTree, float64 -> float32
    want = torch.log(torch.sqrt(d2))[:, None].repeat(1, 3)
    _close(m._scaling.detach().cpu(), want, "scaling from distCUDA2")
    # tensors on the device are taken as they are
    m2 = GaussianModel(3).create_from_pcd(torch.from_numpy(fx["pcd/points"]).to(gpu_device),
                                          torch.from_numpy(fx["pcd/colors"]).to(gpu_device), 2.0)
    assert torch.equal(m2._scaling, m._scaling) and torch.equal(m2._features_dc, m._features_dc)


# ---- 6. reset_opacity -------------------------------------------------------------------------------------------------
def _reset_model(fx, dev, optimizer):
    from mvs_gaussian_splatting_amd import GaussianModel
    m = GaussianModel(0)
    for k, a in GROUP_ATTR.items():
        setattr(m, a, nn.Parameter(torch.from_numpy(fx[f"reset/before/param/{k}"]).to(dev).requires_grad_(True)))
    m.spatial_lr_scale = float(fx["reset/spatial_lr_scale"])
    m.max_radii2D = torch.zeros(m._xyz.shape[0], device=dev)
    m.training_setup(fixture_opt(fx), _optimizer_cls(optimizer))
    for k, a in GROUP_ATTR.items():
        m.optimizer.state[getattr(m, a)] = {"step": torch.tensor(float(fx[f"reset/before/step/{k}"])),
                                            "exp_avg": torch.from_numpy(fx[f"reset/before/exp_avg/{k}"]).to(dev),
                                            "exp_avg_sq": torch.from_numpy(fx[f"reset/before/exp_avg_sq/{k}"]).to(dev)}
    return m


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_reset_opacity_matches_the_reference(gpu_device, optimizer):
    fx = np.load(FIXTURE)
    m = _reset_model(fx, gpu_device, optimizer)
    p, ptr = m._opacity, m._opacity.data_ptr()
    p.grad = torch.ones_like(p)
    m.reset_opacity()
    assert m._opacity is p and p.data_ptr() == ptr and p.grad is None          # in place: same Parameter, grad dropped
    st = m.optimizer.state[p]
    _close(p.detach().cpu(), torch.from_numpy(fx["reset/after/param/opacity"]), "reset values")
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert float(st["step"]) == float(fx["reset/after/step/opacity"]) == 2.0
    for k, a in GROUP_ATTR.items():                                             # the other groups are untouched
        if k != "opacity":
            q = getattr(m, a)
            assert torch.equal(q.detach().cpu(), torch.from_numpy(fx[f"reset/before/param/{k}"]))
            assert torch.equal(m.optimizer.state[q]["exp_avg"].cpu(), torch.from_numpy(fx[f"reset/before/exp_avg/{k}"]))
    # train.py:136-141: gradients everywhere, reset, step -- the opacity group is skipped
    for k, a in GROUP_ATTR.items():
        getattr(m, a).grad = torch.from_numpy(fx[f"reset/grad/{k}"]).to(gpu_device)
    m.reset_opacity()
    m.optimizer.step()
    for k, a in GROUP_ATTR.items():
        q = getattr(m, a)
        st = m.optimizer.state[q]
        assert float(st["step"]) == float(fx[f"reset/after_step/step/{k}"]), k
        _close(q.detach().cpu(), torch.from_numpy(fx[f"reset/after_step/param/{k}"]), f"after step/{k}")
        for key in ("exp_avg", "exp_avg_sq"):
            want = torch.from_numpy(fx[f"reset/after_step/{key}/{k}"])
            if k == "opacity":
                assert torch.equal(st[key].cpu(), want) and not want.any(), key
            else:
                _close(st[key].cpu(), want, f"after step/{key}/{k}")


def _ulp_distance(a, b):
    ia, ib = a.view(torch.int32).long(), b.view(torch.int32).long()
    ia = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return (ia - ib).abs()


def test_reset_opacity_against_torch_ops_on_the_device(gpu_device):
    """Aim: the bits of torch's own sigmoid, min, div, log on the device.  Where a row differs, the kernel's error
    against the float64 value must be at most twice torch's (the project's "2x the float32 oracle" rule)."""
    from mvs_gaussian_splatting_amd import GaussianModel
    g = torch.Generator().manual_seed(3)
    raw = torch.cat([-4.6 + 2.5 * torch.randn(200_001, 1, generator=g), torch.tensor([[-30.0], [-90.0], [0.0], [20.0]])])
    m = GaussianModel(0)
    m._opacity = nn.Parameter(raw.to(gpu_device).requires_grad_(True))
    x = m._opacity.detach().clone()
    o = torch.sigmoid(x)
    c = torch.min(o, torch.ones_like(o) * 0.01)
    want = torch.log(c / (1 - c))                                    # scene/gaussian_model.py:313, utils/general_utils.py:18
    m.reset_opacity()                                                # no optimizer: values only
    got = m._opacity.detach()
    finite = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), finite) and torch.equal(got[~finite], want[~finite])
    ulp = _ulp_distance(got[finite], want[finite])
    print(f"reset_opacity vs torch ops: {int((ulp != 0).sum())} of {ulp.numel()} rows differ, largest distance "
          f"{int(ulp.max())} ulp")
    if int(ulp.max()) != 0:
        c64 = torch.sigmoid(x.double()).clamp(max=0.01)
        ref = torch.log(c64 / (1 - c64))[finite]
        e_got = (got[finite].double() - ref).abs().max()
        e_torch = (want[finite].double() - ref).abs().max()
        print(f"error against float64: kernel {float(e_got):.3e}, torch float32 {float(e_torch):.3e}")
        assert float(e_got) <= 2.0 * float(e_torch)


# ---- 7. the sparsity term ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["some", "one", "none"])
def test_opacity_sparsity_loss_matches_the_reference(gpu_device, case):
    from mvs_gaussian_splatting_amd import opacity_sparsity_loss
    fx = np.load(FIXTURE)
    w = float(fx["sparsity/weight"])
    raw = torch.from_numpy(fx[f"sparsity/{case}/raw"]).to(gpu_device).requires_grad_(True)
    loss, record = opacity_sparsity_loss(raw, w, return_record=True)
    assert loss.dim() == 0 and loss.is_cuda and loss.dtype == torch.float32
    loss.backward()
    n = int(record.view(torch.int32)[1])
    assert n == int(fx[f"sparsity/{case}/n"])
    want = float(fx[f"sparsity/{case}/value_f64"])
    want_grad = torch.from_numpy(fx[f"sparsity/{case}/grad_f64"])
    grad = raw.grad.cpu()
    assert grad.shape == raw.shape and grad.dtype == torch.float32
    if n == 0:
        assert float(loss.detach()) == 0.0 and want == 0.0 and not grad.any()
        return
    rel = abs(float(loss.detach()) - want) / abs(want)
    gerr = float((grad.double() - want_grad).abs().max()) / float(want_grad.abs().max())
    print(f"sparsity/{case}: n {n}, value {float(loss.detach()):.9g} (float64 {want:.12g}, rel {rel:.2e}, bar 1e-6; float32 "
          f"reference {float(fx[f'sparsity/{case}/value_f32']):.9g}); gradient error {gerr:.2e} of max (bar 1e-5)")
    assert rel <= 1e-6
    assert gerr <= 1e-5
    off = want_grad == 0
    assert int((~off).sum()) == n and not grad[off].any()            # exactly zero off the set


def test_opacity_sparsity_loss_zero_weight_scaling_and_determinism(gpu_device):
    from mvs_gaussian_splatting_amd import opacity_sparsity_loss
    fx = np.load(FIXTURE)
    w = float(fx["sparsity/weight"])
    base = torch.from_numpy(fx["sparsity/some/raw"]).to(gpu_device)
    raw = base.clone().requires_grad_(True)
    zero = opacity_sparsity_loss(raw, 0.0)
    assert float(zero) == 0.0 and not zero.requires_grad and zero.is_cuda         # the default configuration: no launch
    assert float(opacity_sparsity_loss(raw, -1.0)) == 0.0
    (opacity_sparsity_loss(raw, w) + 0.0).backward()
    g1, l1 = raw.grad.clone(), opacity_sparsity_loss(raw, w).detach().clone()
    raw.grad = None
    opacity_sparsity_loss(raw, w).backward()
    assert torch.equal(raw.grad, g1) and torch.equal(opacity_sparsity_loss(raw, w).detach(), l1)   # run to run
    # the upstream gradient is a device scalar, read on the device
    raw.grad = None
    k = torch.tensor(3.0, device=gpu_device)
    (opacity_sparsity_loss(raw, w) * k).backward()
    assert torch.equal(raw.grad, (g1 * 3.0)) or float((raw.grad - 3.0 * g1).abs().max()) <= 1e-6 * float(g1.abs().max())
    assert float(raw.grad.abs().max()) > 2.9 * float(g1.abs().max())
    # any length and alignment: the scalar path and the four-row tail agree with the aligned path
    for n in (1, 3, 4001, 3999):
        a = base[:n].clone().requires_grad_(True)
        b = torch.cat([base[:1], base[:n]])[1:].requires_grad_(True)              # 4-byte aligned, not 16
        la, lb = opacity_sparsity_loss(a, w), opacity_sparsity_loss(b, w)
        la.backward()
        lb.backward()
        assert torch.equal(a.grad, b.grad)
        assert abs(float(la.detach()) - float(lb.detach())) <= 1e-6 * abs(float(la.detach()))
        off = torch.sigmoid(a.detach()) >= 0.005
        assert not a.grad[off].any() and bool((a.grad[~off] != 0).all())


# ---- 8. no host round-trip --------------------------------------------------------------------------------------------
def test_sparsity_term_and_reset_run_inside_a_captured_graph(gpu_device):
    """Capture fails on any synchronising call (a read-back, an allocation outside the graph's pool), so capturing the
    forward + backward of the term and reset_opacity shows that they make none; the replay gives the eager bits."""
    from mvs_gaussian_splatting_amd import GaussianModel, opacity_sparsity_loss
    fx = np.load(FIXTURE)
    w = float(fx["sparsity/weight"])
    base = torch.from_numpy(fx["sparsity/some/raw"]).to(gpu_device)
    eager = base.clone().requires_grad_(True)
    le = opacity_sparsity_loss(eager, w)
    le.backward()
    static = base.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # warm-up off the capture, as torch's recipe does
        opacity_sparsity_loss(static, w).backward()
    torch.cuda.current_stream().wait_stream(side)
    static.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = opacity_sparsity_loss(static, w)
        loss.backward()
    static.grad.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), le.detach()) and torch.equal(static.grad, eager.grad)
    with torch.no_grad():                                            # new values, same graph: n changes on the device
        static.copy_(torch.from_numpy(fx["sparsity/one/raw"]).to(gpu_device))
    graph.replay()
    torch.cuda.synchronize()
    assert int((static.grad != 0).sum()) == 1
    assert abs(float(loss) - float(fx["sparsity/one/value_f64"])) <= 1e-6 * float(fx["sparsity/one/value_f64"])

    m = _reset_model(fx, gpu_device, "hip")
    want = _reset_model(fx, gpu_device, "hip")
    want.reset_opacity()
    before = m._opacity.detach().clone()
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        m.reset_opacity()
    with torch.no_grad():
        m._opacity.copy_(before)
        m.optimizer.state[m._opacity]["exp_avg"].fill_(1.0)
    graph2.replay()
    torch.cuda.synchronize()
    assert torch.equal(m._opacity, want._opacity) and not m.optimizer.state[m._opacity]["exp_avg"].any()
    assert isinstance(GaussianModel(0), GaussianModel)


# ---- 9. / 10. the training loop -----------------------------------------------------------------------------------------
def _state(model):
    out = {"active_sh_degree": model.active_sh_degree}
    for grp in model.optimizer.param_groups:
        p = grp["params"][0]
        st = model.optimizer.state.get(p, {})
        out[grp["name"]] = (p.detach().clone(), grp["lr"], float(st["step"]) if "step" in st else None,
                            st.get("exp_avg"), st.get("exp_avg_sq"))
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        out[k] = getattr(model, k).clone()
    return out


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], tuple):
            (pa, lra, sa, ma, va), (pb, lrb, sb, mb, vb) = a[k], b[k]
            assert torch.equal(pa, pb), f"{k}: parameters differ"
            assert lra == lrb and sa == sb, (k, lra, lrb, sa, sb)
            assert (ma is None) == (mb is None), k
            if ma is not None:
                assert torch.equal(ma, mb) and torch.equal(va, vb), f"{k}: moments differ"
        elif torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


RESUME = {
    # densify at 20, 30, 40, the opacity reset at 30
    "plain": dict(dataset=types.SimpleNamespace(white_background=False),
                  opt=dict(densify_from_iter=10, densification_interval=10, opacity_reset_interval=30,
                           densify_until_iter=50)),
    # densify (clone + split over the learned tensors) at 20, the reset at 30, the window closes at 31: from then on
    # every frame renders the learned split of the rows selected by the statistics of iterations 21-30
    "grow_dir_learned_split": dict(
        dataset=types.SimpleNamespace(white_background=False, grow_dir=True, num_dirs=32, continous_dir=False,
                                      grow_distance=True, learn_split_distance=True, learn_split_scale=True,
                                      symmetric_split=False, split_notreinit=False, prob_notreinit=False),
        opt=dict(densify_from_iter=10, densification_interval=20, opacity_reset_interval=30, densify_until_iter=31)),
}


@pytest.mark.parametrize("optimizer", ["hip", "torch"])
@pytest.mark.parametrize("case", sorted(RESUME))
def test_checkpoint_and_resume_is_bit_identical(gpu_device, tmp_path, case, optimizer):
    from mvs_gaussian_splatting_amd.trainer import load_checkpoint, save_checkpoint
    ex = _example()
    K = 20
    dataset = RESUME[case]["dataset"]
    opt = ex.small_opt(2 * K, opacitysparse=0.05, densify_grad_threshold=0.0002, **RESUME[case]["opt"])
    cls = _optimizer_cls(optimizer)
    problem = ex.make_problem(gpu_device, P=1500, W=128, H=80, n_views=4)
    whole = ex.make_model(problem, opt, dataset, optimizer_cls=cls)
    sizes = []
    ex.train(whole, problem, opt, 0, 2 * K, dataset=dataset, on_iteration=lambda it, m: sizes.append(m._xyz.shape[0]))
    assert len(set(sizes)) > 1, "the window must hold a densification that changes the model"
    first = ex.make_model(problem, opt, dataset, optimizer_cls=cls)
    ex.train(first, problem, opt, 0, K, dataset=dataset)
    path = str(tmp_path / f"chkpnt{K}.pth")
    save_checkpoint(first, K, path)
    assert len(first.capture()) == (12 if case == "plain" else 13)
    del first
    resumed = ex.make_model(problem, opt, dataset, optimizer_cls=cls)          # a fresh model, as train.py:37-42
    assert load_checkpoint(resumed, path, opt) == K
    assert isinstance(resumed.optimizer, cls)
    ex.train(resumed, problem, opt, K, 2 * K, dataset=dataset)
    a, b = _state(whole), _state(resumed)
    if case != "plain":
        assert {"dirs_prob", "grow_dist", "split_distance", "split_scale"} <= set(a)
        assert a["split_distance"][3] is not None, "the learned split must have received gradients"
    _assert_same_state(a, b)


def test_the_loop_learns_and_the_ply_round_trips(gpu_device, tmp_path):
    from mvs_gaussian_splatting_amd import GaussianModel
    ex = _example()
    opt = ex.example_opt(200, opacitysparse=0.01)                    # the example's own run: reset at 100, then recovery
    problem = ex.make_problem(gpu_device)
    model = ex.make_model(problem, opt)
    assert model.active_sh_degree == 0
    losses = torch.stack(ex.train(model, problem, opt)).cpu()
    assert torch.isfinite(losses).all()
    start, end = float(losses[:8].mean()), float(losses[-8:].mean())             # one pass over the eight views each
    print(f"loss {start:.5f} -> {end:.5f}, {model._xyz.shape[0]} Gaussians")
    assert end < start
    path = str(tmp_path / "out" / "point_cloud.ply")
    model.save_ply(path)
    again = GaussianModel(3)
    again.load_ply(path)
    assert again.active_sh_degree == again.max_sh_degree == 3
    for a in GROUP_ATTR.values():
        p, q = getattr(model, a), getattr(again, a)
        assert isinstance(q, nn.Parameter) and q.is_cuda and q.requires_grad
        assert torch.equal(p.detach(), q.detach()), a
