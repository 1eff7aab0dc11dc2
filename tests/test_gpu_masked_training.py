"""Training masks inside ``training_iteration`` (trainer.py) on the small synthetic cloud of
``examples/train.py``: a camera without a mask trains by the calls and to the bits it did before, a masked camera's colour
loss is ``masked_l1_dssim_loss`` of the frame, what the mask hides of the target reaches no parameter, and the silhouette
term adds exactly its weighted value and pushes on the opacity of what lies outside the mask.  Also ``Camera``'s resize of a
mask on the GPU against the host restatement of the image resize."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import ingest_restate

sys.path.insert(0, os.path.join(ROOT, "examples"))

pytestmark = pytest.mark.gpu
IT = 3


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


@pytest.fixture(scope="module")
def problem(gpu_device):
    import train as example
    return example.make_problem(gpu_device, P=300, W=64, H=48, n_views=2)


def strip_mask(cam):
    if hasattr(cam, "alpha_mask"):
        delattr(cam, "alpha_mask")


def half_mask(dev, H=48, W=64):
    m = torch.zeros(1, H, W, device=dev)
    m[:, :, :W // 2] = 1.0
    return m


def iterate(problem, cam, opt, gt_image=None):
    """One ``training_iteration`` on a fresh model -> (loss, {group: gradient as the backward left it}, model)."""
    import train as example
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    _, bg, _ = problem
    model = example.make_model(problem, opt)
    grads = {}
    for group in model.optimizer.param_groups:
        group["params"][0].register_hook(lambda gr, name=group["name"]: grads.__setitem__(name, gr.detach().clone()))
    loss = trainer.training_iteration(model, cam, opt, PipelineParams(), bg, IT, cameras_extent=example.CAMERAS_EXTENT,
                                      **({"gt_image": gt_image} if gt_image is not None else {}))
    assert set(grads) == {g["name"] for g in model.optimizer.param_groups}
    return loss, grads, model


def frame(problem, cam, opt, **extra):
    """The frame ``training_iteration`` renders at IT on a fresh model, with the graph it renders it with."""
    import train as example
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    _, bg, _ = problem
    model = example.make_model(problem, opt)
    model.update_learning_rate(IT)
    pkg = trainer.render(cam, model, PipelineParams(), bg, grow_dir=False, densify_grad_threshold=opt.densify_grad_threshold,
                         iteration=IT, opt=opt, continous_dir=False, grow_distance=False, modelcg=None,
                         cameras_extent=example.CAMERAS_EXTENT, **extra)
    return pkg, model


def test_a_camera_without_a_mask_trains_to_the_bits_it_did(gpu_device, problem, monkeypatch):
    import train as example
    from mvs_gaussian_splatting_amd import trainer
    cams, _, _ = problem
    cam = cams[0]
    strip_mask(cam)
    seen, calls, real_render = [], [], trainer.render

    def spy(*args, **kw):
        seen.append(sorted(kw))
        return real_render(*args, **kw)
    monkeypatch.setattr(trainer, "render", spy)
    monkeypatch.setattr(trainer, "masked_l1_dssim_loss", lambda *a, **k: calls.append("colour"))
    monkeypatch.setattr(trainer, "alpha_mask_loss", lambda *a, **k: calls.append("alpha"))
    try:
        bare_loss, bare, _ = iterate(problem, cam, example.small_opt(40))
        cam.alpha_mask = None
        # the new fields away from their defaults: without a mask they are not read
        none_loss, none, _ = iterate(problem, cam, example.small_opt(40, lambda_alpha_mask=0.5, mask_normalize="mask",
                                                                      alpha_mask_mode="l1"))
        default_loss, default, _ = iterate(problem, cam, example.small_opt(40))
    finally:
        strip_mask(cam)
    before = ["cameras_extent", "continous_dir", "densify_grad_threshold", "grow_dir", "grow_distance", "iteration", "modelcg",
              "opt"]
    assert seen == [before] * 3 and not calls
    assert same_bits(bare_loss, none_loss) and same_bits(bare_loss, default_loss)
    for name in bare:
        assert same_bits(bare[name], none[name]) and same_bits(bare[name], default[name]), name


@pytest.mark.parametrize("normalize", ["image", "mask"])
def test_a_masked_cameras_loss_is_the_masked_loss_of_its_frame(gpu_device, problem, normalize):
    import train as example
    from mvs_gaussian_splatting_amd import masked_l1_dssim_loss
    cams, _, _ = problem
    cam = cams[0]
    opt = example.small_opt(40, mask_normalize=normalize)
    try:
        cam.alpha_mask = half_mask(gpu_device)
        loss, grads, _ = iterate(problem, cam, opt)
        image = frame(problem, cam, opt)[0]["render"]
        want = masked_l1_dssim_loss(image.detach(), cam.original_image, cam.alpha_mask, opt.lambda_dssim, normalize)
        plain_loss, _, _ = iterate(problem, cam, example.small_opt(40, mask_photometric=False))
        print(f"[masked training] {normalize}: loss {float(loss):.8f}, on the side {float(want):.8f}, unmasked {float(plain_loss):.8f}")
        assert same_bits(loss, want) and not same_bits(loss, plain_loss)
        # what the mask hides of the target reaches no parameter
        g = torch.Generator().manual_seed(11)
        scrambled = cam.original_image.clone()
        scrambled[:, :, 32:] = torch.rand(3, 48, 32, generator=g).to(gpu_device)
        loss_s, grads_s, _ = iterate(problem, cam, opt, gt_image=scrambled)
        assert same_bits(loss, loss_s)
        for name in grads:
            assert same_bits(grads[name], grads_s[name]), name
        assert any(bool(gr.any()) for gr in grads.values())
        # ... and reaches them all without mask_photometric
        _, grads_p, _ = iterate(problem, cam, example.small_opt(40, mask_photometric=False), gt_image=scrambled)
        _, grads_q, _ = iterate(problem, cam, example.small_opt(40, mask_photometric=False))
        assert not same_bits(grads_p["f_dc"], grads_q["f_dc"])
    finally:
        strip_mask(cam)


@pytest.mark.parametrize("mode", ["bce", "l1"])
def test_the_silhouette_term_adds_its_weighted_value_and_pushes_on_opacity(gpu_device, problem, mode, monkeypatch):
    import train as example
    from mvs_gaussian_splatting_amd import alpha_mask_loss, masked_l1_dssim_loss, trainer
    cams, _, _ = problem
    cam = cams[0]
    weight = 0.25
    opt_off = example.small_opt(40)
    opt_on = example.small_opt(40, lambda_alpha_mask=weight, alpha_mask_mode=mode)
    try:
        cam.alpha_mask = half_mask(gpu_device)
        off_loss, off, _ = iterate(problem, cam, opt_off)
        seen, real_render = [], trainer.render

        def spy(*args, **kw):
            seen.append(dict(kw))
            return real_render(*args, **kw)
        monkeypatch.setattr(trainer, "render", spy)
        on_loss, on, model = iterate(problem, cam, opt_on)
        monkeypatch.setattr(trainer, "render", real_render)
        assert len(seen) == 1 and seen[0].get("return_depth") is True
        pkg, fresh = frame(problem, cam, opt_on, return_depth=True)
        term = alpha_mask_loss(pkg["alpha"].detach(), cam.alpha_mask, mode=mode)
        colour = masked_l1_dssim_loss(pkg["render"].detach(), cam.original_image, cam.alpha_mask, opt_on.lambda_dssim, "image")
        want = colour + torch.tensor(weight, dtype=torch.float32, device=gpu_device) * term
        print(f"[masked training] alpha {mode}: loss {float(off_loss):.8f} without, {float(on_loss):.8f} with; colour "
              f"{float(colour):.8f} + {weight} x term {float(term):.6f}")
        # the colour loss of the frame the term is rendered with, plus exactly the weighted term; the colour image of a
        # frame rendered with its maps is the plain frame's to within an ulp of the loss
        assert float(term) > 0 and same_bits(on_loss, want) and float(on_loss) > float(off_loss)
        assert abs(float(colour) - float(off_loss)) <= 2.0 ** -22 * float(off_loss)
        # Gaussians that project into the mask's zero half get an opacity gradient from the term
        xyz = fresh._xyz.detach()
        hom = torch.cat([xyz, torch.ones_like(xyz[:, :1])], dim=1) @ cam.full_proj_transform
        ndc_x, ndc_y = hom[:, 0] / hom[:, 3].clamp(min=1e-6), hom[:, 1] / hom[:, 3].clamp(min=1e-6)
        outside = (ndc_x > 0.2) & (ndc_x < 0.9) & (ndc_y.abs() < 0.9) & (hom[:, 3] > 0) & (pkg["radii"] > 0)
        assert int(outside.sum()) > 5, "the scene must put Gaussians into the hidden half"
        delta = (on["opacity"] - off["opacity"]).reshape(-1)
        assert bool((delta[outside] != 0).all()) and bool((on["opacity"].reshape(-1)[outside] != 0).all())
        assert float(model.denom.sum()) > 0
    finally:
        strip_mask(cam)


def test_unknown_modes_are_refused_before_anything_is_rendered(gpu_device, problem, monkeypatch):
    import train as example
    from mvs_gaussian_splatting_amd import trainer
    cams, _, _ = problem
    cam = cams[1]
    monkeypatch.setattr(trainer, "render", lambda *a, **k: pytest.fail("rendered"))
    try:
        cam.alpha_mask = half_mask(gpu_device)
        with pytest.raises(ValueError, match="mask_normalize"):
            iterate(problem, cam, example.small_opt(40, mask_normalize="pixels"))
        with pytest.raises(ValueError, match="alpha_mask_mode"):
            iterate(problem, cam, example.small_opt(40, lambda_alpha_mask=0.1, alpha_mask_mode="huber"))
    finally:
        strip_mask(cam)


@pytest.mark.parametrize("size", [(32, 24), (33, 19)], ids=str)
def test_camera_resizes_a_mask_on_the_gpu_as_the_host_restatement_does(gpu_device, size):
    from mvs_gaussian_splatting_amd import scene as sc
    w, h = size
    m = (np.random.default_rng(w * h).integers(0, 2, size=(h, w)) * 255).astype(np.uint8)
    cam = sc.Camera(1, np.eye(3), np.zeros(3), 0.6, 0.5, torch.zeros(3, 48, 64), None, "v", 0, data_device=str(gpu_device),
                    device=str(gpu_device), alpha_mask=m)
    want = torch.from_numpy(np.ascontiguousarray(ingest_restate.resize(m[:, :, None], (64, 48))[:, :, 0])).float() / 255.0
    assert cam.alpha_mask.shape == (1, 48, 64) and cam.alpha_mask.device.type == "cuda"
    assert torch.equal(cam.alpha_mask[0].cpu(), want.clamp(0.0, 1.0))
