"""The fork's grow / learned-split branch on the HIP path (csrc/grow.hip, mvs_gaussian_splatting_amd/grow.py):
the expansion and fold against the fixture recorded from the reference's render() (tests/golden/grow_branch.npz), the
grown frame end to end, the closed gate, and a short training run."""
import types

import numpy as np
import pytest
import torch

from conftest import small_scene
from grow_restate import RECORDED, case_config, case_model, cotangent, restate
from test_grow_host import GOLDEN

pytestmark = pytest.mark.gpu

OPT = types.SimpleNamespace(densify_from_iter=500, densification_interval=100, densify_until_iter=15000,
                            opacity_reset_interval=3000)
FUNCTION_CASES = ["grow_dir", "grow_dir_distance", "continous_dir", "split_distance", "split_scale", "split_both",
                  "grow_split_zero"]


def _activated(ext):
    """The operator inputs the reference builds from the extended raw tensors (getters, scene/gaussian_model.py)."""
    xyz, m2, f_dc, f_rest, op, sc, rot = ext
    return {"means3D": xyz, "means2D": m2, "shs": torch.cat((f_dc, f_rest), dim=1), "opacities": torch.sigmoid(op),
            "scales": torch.exp(sc), "rotations": torch.nn.functional.normalize(rot)}


def _model_ns(m, dev):
    pc = types.SimpleNamespace()
    for k in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"):
        setattr(pc, {"f_dc": "_features_dc", "f_rest": "_features_rest"}.get(k, "_" + k),
                m[k].detach().float().to(dev).requires_grad_(True))
    for k in ("dirs_prob", "conti_dirs", "grow_dist", "split_distance", "split_scale"):
        setattr(pc, "_" + k, m[k].detach().float().to(dev).requires_grad_(True))
    pc.dirs = m["dirs"].float().to(dev)
    pc.xyz_gradient_accum = m["xyz_gradient_accum"].float().to(dev)
    pc.denom = m["denom"].float().to(dev)
    return pc


def _run_function(z, name, dev):
    from mvs_gaussian_splatting_amd import grow
    which, flags, thr, pde = case_config(z, name)
    pc = _model_ns(case_model(z, torch.float32), dev)
    mode = grow.mode_bits(which, flags["grow_dir"], flags["continous_dir"], flags["grow_distance"],
                          types.SimpleNamespace(learn_split_distance=flags["learn_split_distance"],
                                                learn_split_scale=flags["learn_split_scale"]))
    P = pc._xyz.shape[0]
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    noise = torch.from_numpy(z[f"{name}/noise"]).float().to(dev)
    pl, ext = grow.expand(pc, m2, mode, thr, pde, noise=noise if noise.numel() else None)
    act = _activated(ext)
    w = cotangent(int(z[f"{name}/cotangent_seed"]), {k: act[k].shape for k in RECORDED})
    sum((w[k].to(dev) * act[k]).sum() for k in RECORDED).backward()
    leaves = {"xyz": pc._xyz, "f_dc": pc._features_dc, "f_rest": pc._features_rest, "opacity": pc._opacity,
              "scaling": pc._scaling, "rotation": pc._rotation}
    leaves.update({k: getattr(pc, "_" + k) for k in ("dirs_prob", "conti_dirs", "grow_dist", "split_distance",
                                                      "split_scale")})
    grads = {k: (None if v.grad is None else v.grad.detach().cpu()) for k, v in leaves.items()}
    grads["means2D"] = m2.grad.detach().cpu()
    return pl, {k: v.detach().cpu() for k, v in act.items()}, ext, grads


@pytest.mark.parametrize("name", FUNCTION_CASES)
def test_expand_and_fold_against_the_reference(gpu_device, name):
    z = np.load(GOLDEN)
    pl, act, ext, grads = _run_function(z, name, gpu_device)
    P = z["model/xyz"].shape[0]
    assert torch.equal(pl.selected.cpu(), torch.from_numpy(z[f"{name}/selected"]))
    assert act["means3D"].shape[0] == z[f"{name}/ext/means3D"].shape[0] == P + pl.G
    sel = torch.from_numpy(z[f"{name}/selected"])
    which = case_config(z, name)[0]
    # rows the branch computes: the virtual rows' positions; in a split also the moved originals and every scale of both
    computed = {"means3D": torch.cat((sel if which == "split" else torch.zeros(P, dtype=torch.bool),
                                      torch.ones(pl.G, dtype=torch.bool)))}
    computed["scales"] = torch.cat((sel, torch.ones(pl.G, dtype=torch.bool))) if which == "split" else \
        torch.zeros(P + pl.G, dtype=torch.bool)
    for k in RECORDED:
        if k == "means2D":
            continue
        ref = torch.from_numpy(z[f"{name}/ext/{k}"])
        got = act[k]
        rows = computed.get(k, torch.zeros(P + pl.G, dtype=torch.bool))
        # copied rows: the raw tensors are bit copies, so the activations match the reference's getters up to the
        # activation kernels of two torch builds -- compare the raw copies exactly instead
        if k in ("means3D",):
            assert torch.equal(got[~rows], ref[~rows]), f"{name}: copied {k} rows are not bit-identical"
        if rows.any():
            d = (got[rows] - ref[rows]).abs() / ref[rows].abs().clamp(min=float(ref.abs().max()) * 1e-3)
            assert float(d.max()) <= 1e-6, f"{name}: computed {k} rows off by {float(d.max()):.2e}"
        scale = float(ref.abs().max())
        assert float((got - ref).abs().max()) <= 2e-6 * scale, f"{name}: {k}"
    raw_names = ("xyz", "m2", "f_dc", "f_rest", "opacity", "scaling", "rotation")
    src = pl.src.long().cpu()
    for k, t in zip(raw_names, ext):
        if k in ("m2",):
            continue
        t = t.detach().cpu()
        base = torch.from_numpy(z[f"model/{k}"])
        if k in ("f_dc", "f_rest", "opacity", "rotation") or (k == "scaling" and which == "grow"):
            assert torch.equal(t[:P], base) and torch.equal(t[P:], base[src]), f"{name}: {k} copies not bit-identical"
        elif k == "xyz" and which == "grow":
            assert torch.equal(t[:P], base), f"{name}: original positions changed"
        elif which == "split":
            keep = ~sel
            assert torch.equal(t[:P][keep], base[keep]), f"{name}: untouched {k} rows changed"
    none = set(str(s) for s in z[f"{name}/grad_none"])
    for k, g in grads.items():
        if k in none:
            assert g is None, f"{name}: {k} must get no gradient"
            continue
        ref = torch.from_numpy(z[f"{name}/grad/{k}"]).double()
        scale = float(ref.abs().max())
        err = float((g.double() - ref).abs().max()) / scale
        assert err <= 1e-5, f"{name}: gradient of {k} off by {err:.2e}"
    _, _, _, grads2 = _run_function(z, name, gpu_device)
    for k, g in grads.items():
        if g is not None:
            assert torch.equal(g, grads2[k]), f"{name}: backward of {k} is not deterministic"


def test_argmax_handles_many_directions(gpu_device):
    """num_dirs beyond one wave's width: 1000 logits, the maximum in the last stretch, ties to the lowest index."""
    from mvs_gaussian_splatting_amd import grow
    dev = gpu_device
    P, nd = 300, 1000
    g = torch.Generator().manual_seed(3)
    pc = types.SimpleNamespace(_xyz=torch.randn(P, 3, generator=g), _features_dc=torch.randn(P, 1, 3, generator=g),
                               _features_rest=torch.randn(P, 15, 3, generator=g), _opacity=torch.randn(P, 1, generator=g),
                               _scaling=torch.randn(P, 3, generator=g) - 3, _rotation=torch.randn(P, 4, generator=g),
                               _dirs_prob=torch.randn(P, nd, generator=g), dirs=torch.randn(nd, 3, generator=g),
                               xyz_gradient_accum=torch.ones(P, 1), denom=torch.ones(P, 1))
    pc._dirs_prob[:, 990] = 10.0
    pc._dirs_prob[:100, 995] = 10.0                 # tie: 990 wins
    pc._dirs_prob[100:150] = 0.5                    # all tied: 0 wins
    for k, v in list(vars(pc).items()):
        setattr(pc, k, v.to(dev))
    pl, ext = grow.expand(pc, torch.zeros(P, 3, device=dev), 1, 0.5, float("inf"))
    assert pl.G == P
    y = torch.softmax(pc._dirs_prob.double(), dim=1)
    a = torch.full((P,), 990, dtype=torch.long, device=dev)
    a[100:150] = 0
    h = ((1 - y.gather(1, a[:, None])) + y.gather(1, a[:, None])).float()
    want = pc._xyz + (h * pc.dirs[a]) * torch.exp(pc._scaling).max(dim=1, keepdim=True).values
    assert torch.allclose(ext[0][P:], want, rtol=1e-6, atol=1e-6)


# ---- end to end -----------------------------------------------------------------------------------------------------
def _scene(dev, P=3000, seed=0):
    model, cam, bg, target = small_scene(P=P, sh_degree=3, scale=0.05, seed=seed)
    g = torch.Generator().manual_seed(seed + 7)
    model._dirs_prob = torch.randn(P, 128, generator=g)
    model._dirs_prob[: P // 3] = 1.0 / 128
    model._conti_dirs = torch.randn(P, 3, generator=g)
    model._grow_dist = torch.randn(P, 1, generator=g)
    model._split_distance = torch.randn(P, 3, generator=g)
    model._split_scale = torch.randn(P, 1, generator=g)
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams  # noqa: F401
    import math
    n = 128
    i = np.arange(n)
    zz = np.linspace(1 - 1.0 / n, 1.0 / n - 1, n)
    r = np.sqrt(1 - zz * zz)
    th = math.pi * (3 - math.sqrt(5)) * i
    model.dirs = torch.tensor(np.stack([r * np.cos(th), r * np.sin(th), zz], 1), dtype=torch.float32)
    model.denom = torch.randint(0, 4, (P, 1), generator=g).float()
    model.xyz_gradient_accum = torch.rand(P, 1, generator=g) * 0.0006 * model.denom
    model.percent_dense = 0.01
    model.to(dev)
    for k in ("_dirs_prob", "_conti_dirs", "_grow_dist", "_split_distance", "_split_scale", "dirs"):
        setattr(model, k, getattr(model, k).to(dev))
    for p in _leaves(model):
        p.requires_grad_(True)
    cam.to(dev)
    return model, cam, bg.to(dev), target.to(dev)


LEARNED_ATTRS = ("_dirs_prob", "_conti_dirs", "_grow_dist", "_split_distance", "_split_scale")


def _leaves(model):
    return list(model.parameters()) + [getattr(model, k) for k in LEARNED_ATTRS]


VARIANTS = {
    "grow_dir": dict(grow_dir=True, iteration=4000, cg=(False, False)),
    "grow_dir_distance": dict(grow_dir=True, grow_distance=True, iteration=4000, cg=(False, False)),
    "continous_dir": dict(continous_dir=True, grow_distance=True, iteration=4000, cg=(False, False)),
    "split_distance": dict(iteration=10, cg=(True, False)),
    "split_both": dict(iteration=10, cg=(True, True)),
}


def _kwargs(v, extent=2.0):
    kw = {k: v[k] for k in ("grow_dir", "continous_dir", "grow_distance", "iteration") if k in v}
    kw.update(densify_grad_threshold=0.0002, opt=OPT, cameras_extent=extent,
              modelcg=types.SimpleNamespace(learn_split_distance=v["cg"][0], learn_split_scale=v["cg"][1]))
    return kw


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_grown_frame_end_to_end(gpu_device, variant):
    _grown_frame_end_to_end(gpu_device, variant)


@pytest.mark.parametrize("P", [256 * 32 + 1, 256 * 33 + 1])
def test_grown_frame_end_to_end_past_one_scan_line(gpu_device, P):
    """33 and 34 blocks of 256 Gaussians: the plan's block-counter scan moves a whole 32-entry line, and the two counter
    arrays lie nb + 1 = 34 and 35 words apart before the padding."""
    _grown_frame_end_to_end(gpu_device, "grow_dir_distance", P=P)


def _grown_frame_end_to_end(gpu_device, variant, active_sh_degree=None, P=3000):
    """active_sh_degree: None renders at the stored degree; a value below it is set on the model first (the reference
    restatement then runs at that degree too: both read it from the model).  Returns (folded gradients, P)."""
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.rasterizer import GaussianRasterizer
    from mvs_gaussian_splatting_amd.renderer import _settings
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    model, cam, bg, target = _scene(gpu_device, P=P)
    if active_sh_degree is not None:
        model.active_sh_degree = active_sh_degree
    P = model._xyz.shape[0]
    v = VARIANTS[variant]
    kw = _kwargs(v)
    pkg = render(cam, model, PipelineParams(), bg, **kw)
    img = pkg["render"]
    w = torch.rand(img.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float32).to(gpu_device) * 2 - 1
    (img * w).sum().backward()
    got = {k: p.grad.detach().clone() if p.grad is not None else None for k, p in
           zip(("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity") + LEARNED_ATTRS, _leaves(model))}
    got["means2D"] = pkg["viewspace_points"].grad.detach().clone()
    sel = pkg["selected_pts_mask"]
    assert sel is not None and sel.shape == (P,) and 50 < int(sel.sum()) < P
    assert pkg["radii"].shape == (P,) and pkg["visibility_filter"].shape == (P,)
    # the same frame from the torch restatement's extended tensors through the plain operator
    m = {"xyz": model._xyz, "f_dc": model._features_dc, "f_rest": model._features_rest, "opacity": model._opacity,
         "scaling": model._scaling, "rotation": model._rotation, "dirs": model.dirs,
         "xyz_gradient_accum": model.xyz_gradient_accum, "denom": model.denom}
    m.update({k[1:]: getattr(model, k) for k in LEARNED_ATTRS})
    for p in _leaves(model):
        p.grad = None
    flags = {"grow_dir": v.get("grow_dir", False), "continous_dir": v.get("continous_dir", False),
             "grow_distance": v.get("grow_distance", False), "learn_split_distance": v["cg"][0],
             "learn_split_scale": v["cg"][1]}
    which = "split" if v["cg"][0] or v["cg"][1] else "grow"
    m2 = torch.zeros(P, 3, device=gpu_device, requires_grad=True)
    ext, sel_r = restate(m, which, flags, 0.0002, float(np.float32(0.01 * 2.0)), m2)
    assert torch.equal(sel_r, sel)
    st = _settings(cam, model, PipelineParams(), bg, 1.0)
    ref_img, ref_radii = GaussianRasterizer(st)(means3D=ext["means3D"], means2D=ext["means2D"], shs=ext["shs"],
                                                opacities=ext["opacities"], scales=ext["scales"],
                                                rotations=ext["rotations"])
    (ref_img * w).sum().backward()
    assert torch.equal(ref_radii[:P], pkg["radii"])
    assert float((img - ref_img).detach().abs().max()) <= 1e-5
    ref = {k: p.grad for k, p in zip(got, _leaves(model))}
    ref["means2D"] = m2.grad
    for k, g in got.items():
        r = ref[k]
        if r is None:
            assert g is None, f"{variant}: {k} must get no gradient"
            continue
        assert g is not None, f"{variant}: {k} got no gradient"
        scale = float(r.abs().max())
        err = float((g - r).abs().max()) / scale if scale > 0 else float(g.abs().max())
        assert err <= 1e-4, f"{variant}: gradient of {k} off by {err:.2e}"
    assert st.sh_degree == model.active_sh_degree
    return got, P


@pytest.fixture()
def fresh_state(monkeypatch):
    from mvs_gaussian_splatting_amd import rasterizer
    rasterizer.synchronize_counts()
    rasterizer._states.clear()
    monkeypatch.setattr(rasterizer, "_sync_free_value", rasterizer.SYNC_VERIFIED)
    yield rasterizer
    rasterizer._states.clear()


def test_closed_gate_is_the_plain_frame(gpu_device, fresh_state):
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    rz = fresh_state
    model, cam, bg, target = _scene(gpu_device)
    pipe = PipelineParams()
    closed = [dict(grow_dir=True, iteration=3000), dict(grow_dir=True, iteration=None),
              dict(continous_dir=True, iteration=20000)]

    def frame(**kw):
        for p in _leaves(model):
            p.grad = None
        pkg = render(cam, model, pipe, bg, **kw)
        (pkg["render"] * target).sum().backward()
        return pkg, [p.grad.clone() for p in model.parameters()] + [pkg["viewspace_points"].grad.clone()]

    pkg0, g0 = frame()
    for c in closed:
        for p in _leaves(model):
            p.grad = None
        kw = dict(c, densify_grad_threshold=0.0002, opt=OPT, cameras_extent=2.0,
                  modelcg=types.SimpleNamespace(learn_split_distance=False, learn_split_scale=False))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            pkg = render(cam, model, pipe, bg, **kw)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        ctx = pkg["render"].grad_fn
        assert ctx.frame_pending is None and ctx.layout[1] == model._xyz.shape[0]
        assert ctx.layout == pkg0["render"].grad_fn.layout or ctx.layout[0] >= rz.frame_counts(pkg0["render"])[0]
        assert pkg["selected_pts_mask"] is None
        (pkg["render"] * target).sum().backward()
        g1 = [p.grad.clone() for p in model.parameters()] + [pkg["viewspace_points"].grad.clone()]
        for p in _leaves(model):
            p.grad = None
        assert torch.equal(pkg["render"], pkg0["render"]) and torch.equal(pkg["radii"], pkg0["radii"])
        for a, b in zip(g0, g1):
            assert torch.equal(a, b)
        assert all(getattr(model, k).grad is None for k in LEARNED_ATTRS)
    # G = 0 (threshold above every gradient): the plain frame's image
    pkg, _ = frame(grow_dir=True, iteration=4000, densify_grad_threshold=1.0, opt=OPT, cameras_extent=2.0)
    assert torch.equal(pkg["render"], pkg0["render"]) and torch.equal(pkg["radii"], pkg0["radii"])
    assert int(pkg["selected_pts_mask"].sum()) == 0
    # no_grad forward (training_report)
    with torch.no_grad():
        pkg = render(cam, model, pipe, bg, **_kwargs(VARIANTS["grow_dir"]))
    assert pkg["radii"].shape == (model._xyz.shape[0],)
    # the case the reference cannot run raises before anything is rendered or remembered
    states = dict(rz._states)
    before = [p.detach().clone() for p in _leaves(model)]
    with pytest.raises(ValueError, match="__init__.py:181"):
        render(cam, model, pipe, bg, grow_dir=True, iteration=4000, densify_grad_threshold=0.0002, opt=OPT,
               cameras_extent=2.0, modelcg=types.SimpleNamespace(learn_split_distance=True, learn_split_scale=False))
    assert dict(rz._states) == states
    assert all(torch.equal(a, b) for a, b in zip(before, _leaves(model)))
    with pytest.raises(ValueError, match="SH"):
        render(cam, model, pipe, bg, override_color=torch.rand(model._xyz.shape[0], 3, device=gpu_device),
               **_kwargs(VARIANTS["grow_dir"]))


def test_training_steps_with_the_gate_open(gpu_device, fresh_state):
    from mvs_gaussian_splatting_amd import render, add_densification_stats
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    rz = fresh_state
    model, cam, bg, target = _scene(gpu_device)
    P = model._xyz.shape[0]
    pipe = PipelineParams()
    pipe.fuse_densify_stats = True          # must be ignored on grown frames
    pkg = render(cam, model, pipe, bg)      # the plain model's state
    (pkg["render"] - target).abs().mean().backward()
    plain_key = [k for k in rz._states]
    assert len(plain_key) == 1
    opt = torch.optim.Adam(_leaves(model), lr=1e-3)
    Gs, n_states = set(), []
    for it in range(30):
        opt.zero_grad(set_to_none=True)
        pkg = render(cam, model, pipe, bg, **_kwargs(VARIANTS["grow_dir_distance"]))
        loss = (pkg["render"] - target).abs().mean()
        assert torch.isfinite(loss)
        loss.backward()
        sel = pkg["selected_pts_mask"]
        Gs.add(int(sel.sum()))
        for k in ("_dirs_prob", "_grow_dist"):
            g = getattr(model, k).grad
            assert g is not None and torch.isfinite(g).all()
            assert float(g[~sel].abs().max()) == 0.0
            assert float(g[sel].abs().sum()) > 0.0
        ctx = pkg["render"].grad_fn
        if it > 0:      # issued from the shared grown-frame capacity: laid out for (capacity, P + G), no read-back
            assert ctx.frame_pending is None and ctx.layout[1] == P + int(sel.sum()) and ctx.layout[0] >= ctx.counts[0]
        add_densification_stats(model, pkg["viewspace_points"], pkg["radii"])
        opt.step()
        with torch.no_grad():                 # let the selection move from frame to frame
            model.xyz_gradient_accum.mul_(0.9)
        n_states.append(len(rz._states))
    assert len(Gs) > 3, Gs
    assert max(n_states) == 2 and plain_key[0] in rz._states
    W, H = cam.image_width, cam.image_height
    assert rz.reissued_frames(gpu_device, P, W, H, grown=True) == 0
    assert rz.last_counts(gpu_device, P, W, H, grown=True)[0] > 0
