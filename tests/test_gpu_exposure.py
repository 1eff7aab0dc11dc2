"""Per-image exposure compensation on the MI355X (mvs_gaussian_splatting_amd/exposure.py, csrc/exposure.hip) against the
float64 restatement of tests/exposure_restate.py, and through the optimizer, the trainer, the renderer and ``Scene``.

Bars, from the rounding count with u = 2^-24 (not measured):
    y   |y - y64|   <= 5u (sum_k |x_k A_kc| + |A_c3|)     three products and three sums: four roundings on the longest path
    dx  |dx - dx64| <= 4u sum_c |A_kc g_c|                 three roundings on the longest path
    dA  |dA - dA64| <= 2u sum_p |term|                     one rounding to float32 after a double accumulation
The identity exposure is exact: y == x and dx == g as int32 bits; dA is the same bits from call to call.
"""
import os
import random
import sys
import types

import pytest
import torch

from exposure_restate import A_TRUE, U, backward64, forward64

pytestmark = pytest.mark.gpu
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SHAPES = {"sub_wave": (5, 7),            # 35 pixels: less than one wave
          "ragged": (67, 131),           # 8777 pixels: 35 blocks, the last one ragged
          "over_the_cap": (270, 480)}    # 129600 pixels: 507 blocks' worth for 480 slots: strides, and slots per lane
_CASES = {}


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _case(dev, shape, which):
    """x, gt, A and one forward + backward through the HIP L1 loss, computed once per (shape, exposure) and shared:
    y, g = dL/dy, dx, dA from the operator; the float64 restatement of each with its scale."""
    key = (shape, which)
    if key in _CASES:
        return _CASES[key]
    from mvs_gaussian_splatting_amd import apply_exposure, l1_loss
    H, W = SHAPES[shape]
    torch.manual_seed(0)
    x = torch.rand(3, H, W).to(dev)
    a_true = torch.tensor(A_TRUE)
    gt = forward64(x, a_true)[0].to(torch.float32).to(dev)
    A = (torch.eye(3, 4) if which == "identity" else a_true + 0.01).to(dev)
    xg, Ag = x.clone().requires_grad_(True), A.clone().requires_grad_(True)
    y = apply_exposure(xg, Ag)
    y.retain_grad()
    l1_loss(y, gt).backward()
    torch.cuda.synchronize()
    c = types.SimpleNamespace(x=x, gt=gt, A=A, y=y.detach(), g=y.grad.clone(), dx=xg.grad.clone(), dA=Ag.grad.clone())
    c.y64, c.y_mag = forward64(x, A)
    c.dx64, c.dx_mag, c.dA64, c.dA_mag = backward64(x, A, c.g)
    _CASES[key] = c
    return c


@pytest.mark.parametrize("which", ["identity", "offset"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_forward_and_gradients_meet_the_rounding_bars(gpu_device, shape, which):
    c = _case(gpu_device, shape, which)
    assert c.y.shape == c.x.shape and c.dx.shape == c.x.shape and c.dA.shape == (3, 4)
    assert c.g.abs().max() > 0
    for name, got, want, mag, k in (("y", c.y, c.y64, c.y_mag, 5), ("dx", c.dx, c.dx64, c.dx_mag, 4),
                                    ("dA", c.dA, c.dA64, c.dA_mag, 2)):
        err = (got.cpu().double() - want).abs()
        worst = float((err / (U * mag).clamp(min=1e-300)).max())
        print(f"{shape} {which} {name}: worst error {worst:.3f} u * scale (bar {k})")
        assert (err <= k * U * mag).all(), (name, worst)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_identity_exposure_changes_no_bit(gpu_device, shape):
    c = _case(gpu_device, shape, "identity")
    assert torch.isfinite(c.x).all()
    assert torch.equal(_bits(c.y), _bits(c.x)), "y differs from x under the identity exposure"
    assert torch.equal(_bits(c.dx), _bits(c.g)), "dx differs from g under the identity exposure"


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_dA_is_reproducible_and_each_gradient_can_be_left_out(gpu_device, shape):
    from mvs_gaussian_splatting_amd import apply_exposure
    c = _case(gpu_device, shape, "offset")
    # a second backward of the same inputs: the same bits
    xg, Ag = c.x.clone().requires_grad_(True), c.A.clone().requires_grad_(True)
    apply_exposure(xg, Ag).backward(c.g)
    assert torch.equal(_bits(Ag.grad), _bits(c.dA)) and torch.equal(_bits(xg.grad), _bits(c.dx))
    # dx = NULL: the image needs no gradient
    A_only = c.A.clone().requires_grad_(True)
    y = apply_exposure(c.x, A_only)
    assert torch.equal(_bits(y), _bits(c.y))
    y.backward(c.g)
    assert torch.equal(_bits(A_only.grad), _bits(c.dA))
    # dA = NULL: the exposure needs no gradient
    x_only = c.x.clone().requires_grad_(True)
    apply_exposure(x_only, c.A).backward(c.g)
    assert torch.equal(_bits(x_only.grad), _bits(c.dx))
    assert not apply_exposure(c.x, c.A).requires_grad


def test_a_permuted_image_is_made_contiguous(gpu_device):
    from mvs_gaussian_splatting_amd import apply_exposure
    c = _case(gpu_device, "ragged", "offset")
    hwc = c.x.permute(1, 2, 0).contiguous()                          # the same image stored [H,W,3]
    xp = hwc.permute(2, 0, 1).requires_grad_(True)
    assert not xp.is_contiguous() and torch.equal(xp, c.x)
    Ag = c.A.clone().requires_grad_(True)
    y = apply_exposure(xp, Ag)
    assert y.is_contiguous() and torch.equal(_bits(y), _bits(c.y))
    y.backward(c.g)
    assert torch.equal(_bits(xp.grad), _bits(c.dx)) and torch.equal(_bits(Ag.grad), _bits(c.dA))


def test_arguments_are_checked(gpu_device):
    from mvs_gaussian_splatting_amd import _lib, apply_exposure
    x, A = torch.rand(3, 5, 7, device=gpu_device), torch.eye(3, 4, device=gpu_device)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        apply_exposure(x, A.cpu())
    with pytest.raises(TypeError):
        apply_exposure(x.double(), A)
    with pytest.raises(ValueError):
        apply_exposure(x[:2], A)
    with pytest.raises(ValueError):
        apply_exposure(x, A[:, :3])


def _torch_apply(x, A):
    """The definition on torch's elementwise ops, left to right."""
    return torch.stack([x[0] * A[0, c] + x[1] * A[1, c] + x[2] * A[2, c] + A[c, 3] for c in range(3)])


def test_adam_on_the_exposure_follows_torch(gpu_device):
    """3x48x64 from the identity, lr 0.01, eps 1e-8, three steps: this package's Adam over the HIP operator and loss
    against torch.optim.Adam over torch ops.  Every gradient entry of these inputs is >= 6e-3 in magnitude in float64
    (asserted below), far above eps, so the comparison hides no entry.  Bar: |dA| <= 1e-3 lr after each step."""
    from mvs_gaussian_splatting_amd import apply_exposure, l1_loss, optim
    lr = 0.01
    torch.manual_seed(0)
    x = torch.rand(3, 48, 64).to(gpu_device)
    gt = forward64(x, torch.tensor(A_TRUE))[0].to(torch.float32).to(gpu_device)
    A_hip = torch.nn.Parameter(torch.eye(3, 4, device=gpu_device))
    A_ref = torch.nn.Parameter(torch.eye(3, 4, device=gpu_device))
    hip = optim.Adam([A_hip], lr=lr, eps=1e-8)
    ref = torch.optim.Adam([A_ref], lr=lr, eps=1e-8)
    losses = []
    for step in range(3):
        loss = l1_loss(apply_exposure(x, A_hip), gt)
        loss.backward()
        y64 = forward64(x, A_hip)[0]
        g64 = torch.sign(y64 - gt.cpu().double()) / y64.numel()
        smallest = float(backward64(x, A_hip, g64)[2].abs().min())
        assert smallest >= 6e-3, (step, smallest)
        hip.step()
        hip.zero_grad(set_to_none=True)
        (_torch_apply(x, A_ref) - gt).abs().mean().backward()
        ref.step()
        ref.zero_grad(set_to_none=True)
        losses.append(float(loss))
        diff = float((A_hip.detach() - A_ref.detach()).abs().max())
        print(f"step {step + 1}: loss {losses[-1]:.6f}  max |A_hip - A_ref| {diff:.3e} (bar {1e-3 * lr:.1e})  "
              f"smallest |dA64| {smallest:.3e}")
        assert diff <= 1e-3 * lr, (step, diff)
    assert losses[0] > losses[1] > losses[2], losses
    assert not torch.equal(A_hip.detach().cpu(), torch.eye(3, 4))


# ---- trainer, renderer, checkpoints, Scene ----------------------------------------------------------------------------
NAMES = ["view_a", "view_b", "view_c"]
SPLIT = types.SimpleNamespace(white_background=False, grow_dir=False, continous_dir=False, grow_distance=False,
                              learn_split_distance=True, learn_split_scale=True, symmetric_split=False,
                              split_notreinit=False, prob_notreinit=False)


def _example():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train as example
    return example


@pytest.fixture(scope="module")
def problem(gpu_device):
    """The synthetic scene of the training-loop tests (examples/train.py), small, with three named cameras."""
    cams, bg, cloud = _example().make_problem(gpu_device, P=1500, W=128, H=80, n_views=3)
    for cam, name in zip(cams, NAMES):
        cam.image_name = name
    return cams, bg, cloud


def _model(problem, opt, exposures, dataset=None):
    model = _example().make_model(problem, opt, dataset)
    if exposures:
        model.setup_exposures(NAMES)
        model.training_setup(opt)
    return model


def _run(model, problem, opt, first, last, train_exposure, dataset=None):
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from mvs_gaussian_splatting_amd.trainer import training_iteration
    ex = _example()
    cams, bg, _ = problem
    used = []
    for iteration in range(first + 1, last + 1):
        torch.manual_seed(iteration)
        cam = cams[iteration % len(cams)]
        used.append(cam.image_name)
        training_iteration(model, cam, opt, PipelineParams(), bg, iteration, dataset=dataset,
                           cameras_extent=ex.CAMERAS_EXTENT, train_exposure=train_exposure)
    return used


def _state(model):
    out = {}
    for grp in model.optimizer.param_groups:
        p = grp["params"][0]
        st = model.optimizer.state[p]
        out[grp["name"]] = (p.detach().clone(), float(st["step"]), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        out[k] = (getattr(model, k).clone(),)
    return out


def _exposure_state(model):
    st = model.exposure_optimizer.state[model._exposure]
    return model._exposure.detach().clone(), float(st["step"]), st["exp_avg"].clone(), st["exp_avg_sq"].clone()


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        for va, vb in zip(a[k], b[k]):
            assert (torch.equal(_bits(va), _bits(vb)) if torch.is_tensor(va) else va == vb), k


def test_zero_rates_train_exactly_as_without_exposures(gpu_device, problem):
    ex = _example()
    zero = dict(exposure_lr_init=0.0, exposure_lr_final=0.0, exposure_lr_delay_steps=0, exposure_lr_delay_mult=0.0)
    opt_on, opt_off = ex.small_opt(40, **zero), ex.small_opt(40)
    with_exp = _model(problem, opt_on, True)
    _run(with_exp, problem, opt_on, 0, 2, True)
    without = _model(problem, opt_off, False)
    _run(without, problem, opt_off, 0, 2, False)
    assert without.exposure_optimizer is None and len(without.capture()) == 12
    _assert_same(_state(with_exp), _state(without))
    eye = torch.eye(3, 4, device=gpu_device)
    assert all(torch.equal(_bits(row), _bits(eye)) for row in with_exp._exposure.detach())
    assert with_exp.exposure_optimizer.state[with_exp._exposure]["exp_avg"].abs().max() > 0    # it did receive gradients


def test_only_the_frames_row_moves(gpu_device, problem):
    ex = _example()
    opt = ex.small_opt(40)
    model = _model(problem, opt, True)
    used = _run(model, problem, opt, 0, 1, True)
    row = model.exposure_mapping[used[0]]
    eye = torch.eye(3, 4, device=gpu_device)
    for i in range(len(NAMES)):
        same = torch.equal(_bits(model._exposure[i]), _bits(eye))
        assert same == (i != row), (i, row)
    assert float((model._exposure[row].detach() - eye).abs().max()) <= 0.01 * (1 + 1e-6)   # one Adam step: at most lr
    assert model._exposure.grad is None


def test_checkpoint_and_resume_keeps_the_exposures_bit_for_bit(gpu_device, problem, tmp_path):
    from mvs_gaussian_splatting_amd.trainer import load_checkpoint, save_checkpoint
    ex = _example()
    opt = ex.small_opt(40)
    whole = _model(problem, opt, True)
    _run(whole, problem, opt, 0, 4, True)
    first = _model(problem, opt, True)
    _run(first, problem, opt, 0, 2, True)
    path = str(tmp_path / "chkpnt2.pth")
    save_checkpoint(first, 2, path)
    assert len(first.capture()) == 13 and "exposure_mapping" in first.capture()[12]
    del first
    resumed = _model(problem, opt, True)
    assert load_checkpoint(resumed, path, opt) == 2
    assert resumed.exposure_mapping == whole.exposure_mapping
    _run(resumed, problem, opt, 2, 4, True)
    _assert_same({"exposure": _exposure_state(whole)}, {"exposure": _exposure_state(resumed)})
    _assert_same(_state(whole), _state(resumed))          # the existing checkpoint test's bar: the run is reproducible
    with pytest.raises(ValueError, match="exposures"):
        load_checkpoint(_model(problem, opt, False), path, opt)


def test_render_with_trained_exposure_on_every_kind_of_frame(gpu_device, problem):
    from mvs_gaussian_splatting_amd import apply_exposure, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    ex = _example()
    cams, bg, _ = problem
    opt = ex.small_opt(40, densify_grad_threshold=0.0002)
    model = _model(problem, opt, True, SPLIT)
    with torch.no_grad():
        model._exposure[1] = (torch.tensor(A_TRUE) + 0.01).to(gpu_device)
    cam, A = cams[1], model._exposure[1].detach()
    pipe = PipelineParams()
    with torch.no_grad():
        # a plain frame, with the maps
        plain = render(cam, model, pipe, bg, return_depth=True)
        exp = render(cam, model, pipe, bg, return_depth=True, use_trained_exp=True)
        assert torch.equal(_bits(exp["render"]), _bits(apply_exposure(plain["render"], A)))
        assert not torch.equal(exp["render"], plain["render"])
        for k in ("depth", "invdepth", "alpha", "radii", "visibility_filter"):
            assert torch.equal(exp[k], plain[k]), k
        # a frame of the open learned-split branch: statistics that select rows, as after some training
        g = torch.Generator().manual_seed(5)
        P = model._xyz.shape[0]
        model.denom = torch.ones(P, 1, device=gpu_device)
        model.xyz_gradient_accum = (torch.rand(P, 1, generator=g) * 0.0006).to(gpu_device)
        kw = dict(densify_grad_threshold=opt.densify_grad_threshold, iteration=5, opt=opt, modelcg=SPLIT,
                  cameras_extent=ex.CAMERAS_EXTENT)
        torch.manual_seed(9)
        grown = render(cam, model, pipe, bg, **kw)
        torch.manual_seed(9)
        grown_exp = render(cam, model, pipe, bg, use_trained_exp=True, **kw)
        assert grown["selected_pts_mask"] is not None and int(grown["selected_pts_mask"].sum()) > 0
        assert not torch.equal(grown["render"], plain["render"])
        assert torch.equal(_bits(grown_exp["render"]), _bits(apply_exposure(grown["render"], A)))
        assert torch.equal(grown_exp["selected_pts_mask"], grown["selected_pts_mask"])
    # the getter path
    slow = types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False, fuse_activations=False)
    with torch.no_grad():
        a = render(cam, model, slow, bg)["render"]
        b = render(cam, model, slow, bg, use_trained_exp=True)["render"]
    assert torch.equal(_bits(b), _bits(apply_exposure(a, A)))
    # a camera without an exposure is an error that names it
    cam.image_name = "nobody"
    try:
        with pytest.raises(KeyError, match="nobody"):
            render(cam, model, pipe, bg, use_trained_exp=True)
    finally:
        cam.image_name = NAMES[1]
    model_plain = _model(problem, opt, False)
    with pytest.raises(ValueError, match="setup_exposures"):
        _run(model_plain, problem, opt, 0, 1, True)


def test_scene_saves_and_loads_the_trained_exposures(gpu_device, tmp_path):
    pytest.importorskip("PIL", reason="the scene's images are PNG files")
    from test_gpu_scene import write_colmap_scene
    from mvs_gaussian_splatting_amd import GaussianModel, ModelParams, Scene, apply_exposure, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from mvs_gaussian_splatting_amd.trainer import training_iteration
    ex = _example()
    src, out = str(tmp_path / "scene"), str(tmp_path / "out")
    write_colmap_scene(src, gpu_device)
    dataset = ModelParams(source_path=src, model_path=out, resolution=4)
    opt = ex.small_opt(30)
    model = GaussianModel(dataset.sh_degree)
    random.seed(0)
    torch.manual_seed(0)
    scene = Scene(dataset, model)
    cams = scene.getTrainCameras()
    model.setup_exposures([c.image_name for c in cams])
    model.training_setup(opt)
    bg, pipe = torch.zeros(3, device=gpu_device), PipelineParams()
    for iteration in (1, 2, 3):
        torch.manual_seed(iteration)
        training_iteration(model, cams[iteration], opt, pipe, bg, iteration, dataset=dataset,
                           cameras_extent=scene.cameras_extent, train_exposure=True)
    scene.save(3)
    assert os.path.exists(os.path.join(out, "point_cloud", "iteration_3", "exposure.json"))
    again = GaussianModel(dataset.sh_degree)
    scene2 = Scene(dataset, again, load_iteration=3, shuffle=False, defer_cameras=True)
    assert scene2.loaded_iter == 3 and set(again.pretrained_exposures) == set(model.exposure_mapping)
    eye = torch.eye(3, 4, device=gpu_device)
    moved = 0
    for name, row in model.exposure_mapping.items():
        got = again.pretrained_exposures[name]
        assert got.device == model._exposure.device and torch.equal(_bits(got), _bits(model._exposure[row])), name
        moved += int(not torch.equal(got, eye))
    assert moved == 3
    # the loaded model renders the view with its loaded exposure
    view = cams[1]
    model.active_sh_degree = model.max_sh_degree           # load_ply activates every SH degree
    with torch.no_grad():
        a = render(view, model, pipe, bg, use_trained_exp=True)["render"]
        b = render(view, again, pipe, bg, use_trained_exp=True)["render"]
        c = apply_exposure(render(view, again, pipe, bg)["render"], again.pretrained_exposures[view.image_name])
    assert torch.equal(a, b) and torch.equal(b, c)
    # a model trained without exposures leaves no file, and loading it sets nothing
    plain = GaussianModel(dataset.sh_degree)
    out2 = str(tmp_path / "out2")
    scene3 = Scene(ModelParams(source_path=src, model_path=out2, resolution=4), plain, defer_cameras=True)
    scene3.save(1)
    assert not os.path.exists(os.path.join(out2, "point_cloud", "iteration_1", "exposure.json"))
