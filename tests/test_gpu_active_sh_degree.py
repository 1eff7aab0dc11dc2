"""The HIP path at an ACTIVE SH degree below the degree the storage was sized for (GsrParams.D < degree of M).

The reference starts every model at ``active_sh_degree = 0`` with degree-3 storage (``scene/gaussian_model.py:47``) and
raises the degree every 1000 iterations (``train.py:75-76``): the first 3000 iterations of every training run, and every
checkpoint saved in them, are rendered in this state.  The kernels have code of their own for it (csrc/preprocess.hip:
the zero fill of the inactive gradient rows in an LDS stage that has just served as scratch, the guards in front of the
f_rest loads, the d rgb / d direction chain cut off below degree 3), and everything that carries ``sh_degree`` along
(capacity state of the sync-free forward, grown frames, captured graphs, fused densification statistics, the training
example) has to carry a degree that changes.

Truth is the float64 oracle at the same (stored, active) pair, as for the other rasterizer tests, at the bars those tests
use (tests/grad_util.py; nothing new).  On top of the max-norm comparisons, which garbage of 1e-6 of a tensor's largest
element would pass: the gradient rows of the inactive coefficients are EXACT zeros for every Gaussian, and nothing the
operator returns depends on the inactive coefficients' values (they may be 1e30 or NaN), bit for bit.
"""
import os
import sys

import pytest
import torch

from conftest import make_settings, small_scene
from test_gpu_parity import _forward_stages_match_oracle, _fused_raw_parameter_path, _masked_grad_parity

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "examples"))

STORED_ACTIVE = [(3, 0), (3, 1), (3, 2), (2, 0), (2, 1), (1, 0)]
# scene sizes of test_forward_stages_match_oracle, by stored degree (odd sizes: partial tiles; P is no multiple of 64)
FORWARD_SCENE = {3: (3000, 320, 176), 2: (800, 64, 48), 1: (1500, 97, 131)}
BG = (0.3, 0.1, 0.2)


def _n_rest(active):
    """Rows of f_rest that degree `active` reads."""
    return (active + 1) ** 2 - 1


def _assert_inactive_rows_zero(g_rest, active, label):
    """g_rest: dL/d f_rest [P, n, 3] (row k of it is coefficient k + 1).  Every row above the active degree is an exact
    zero for all P Gaussians; the active ones are not all zero."""
    used = _n_rest(active)
    assert g_rest.dim() == 3 and g_rest.shape[1] > used, f"{label}: nothing is inactive in {tuple(g_rest.shape)}"
    bad = int(torch.count_nonzero(g_rest[:, used:, :]))
    assert bad == 0, (f"{label}: {bad} non-zero element(s) in the gradient of the SH coefficients above degree {active}; "
                      f"largest {float(g_rest[:, used:, :].abs().max()):.3e}")
    if used:
        assert int(torch.count_nonzero(g_rest[:, :used, :])) > 0, f"{label}: the active rows carry no gradient"


def _assert_three_kinds(radii, grads, label):
    """The backward treats three kinds of Gaussian differently (culled; visible but without a gradient row; visible with
    rows) and a partial last wave: the scene must have all of them.  A Gaussian without rows has every gradient zero."""
    P = radii.numel()
    assert P % 64 != 0, "the last wave must be partial"
    vis = radii.cpu() > 0
    silent = (grads["opacity"].reshape(P) == 0) & (grads["means2D"].reshape(P, -1) == 0).all(dim=1) & \
        (grads["f_dc"].reshape(P, -1) == 0).all(dim=1)
    n = {"culled": int((~vis).sum()), "visible without rows": int((vis & silent).sum()),
         "visible with rows": int((vis & ~silent).sum())}
    assert all(v > 0 for v in n.values()), f"{label}: the scene lacks a kind of Gaussian: {n}"
    assert not bool((~vis & ~silent).any()), f"{label}: a culled Gaussian received a gradient"
    return n


# ---- 1. forward stages, operator / getter path -------------------------------------------------------------------------
@pytest.mark.parametrize("stored,active,mode", [(s, a, m) for s, a in STORED_ACTIVE for m in ((0, 1) if s == 3 else (0,))],
                         ids=lambda v: str(v))
def test_forward_stages_match_oracle_below_the_stored_degree(gpu_device, stored, active, mode):
    P, w, h = FORWARD_SCENE[stored]
    assert P % 64 != 0
    _forward_stages_match_oracle(gpu_device, stored, active, P, w, h, mode)


# ---- 2. + 3. backward vs float64 autograd, operator path; inactive rows exact zeros ---------------------------------------
@pytest.mark.parametrize("stored,active", STORED_ACTIVE)
def test_backward_matches_fp64_oracle_below_the_stored_degree(gpu_device, stored, active):
    """The scene of test_backward_matches_fp64_oracle (2500 = 39 * 64 + 4 Gaussians) through the masked run and the
    all-pixel runs of _masked_grad_parity.  At degree 0 f_rest is read by nothing: reference and HIP gradient exactly zero."""
    model, cam, _, target = small_scene(P=2500, sh_degree=stored, width=208, height=120, scale=0.06)
    bg = torch.tensor(BG)
    label = f"backward stored degree {stored}, active {active}"
    seen = []

    def check(got, ref, aux):
        assert got["f_rest"].shape == (2500, (stored + 1) ** 2 - 1, 3)
        _assert_inactive_rows_zero(got["f_rest"], active, label)          # rows (active + 1)^2 .. of dL_dshs
        _assert_inactive_rows_zero(ref["f_rest"], active, label + " (oracle)")
        seen.append(_assert_three_kinds(aux["radii"], got, label))

    _masked_grad_parity(gpu_device, model, cam, bg, target, active, label,
                        must_be_zero=("f_rest",) if active == 0 else (), check=check)
    assert len(seen) >= 2                                                 # the masked run and at least one all-pixel run
    print(f"[kinds] {label}: {seen[0]}")


# ---- 4. fused raw-parameter path (render(), split f_dc / f_rest) ----------------------------------------------------------
@pytest.mark.parametrize("active", [0, 1, 2])
def test_fused_raw_parameter_path_below_the_stored_degree(gpu_device, active):
    """test_fused_raw_parameter_path_matches_unfused_and_oracle at active_sh_degree < 3: at degree 0 this is "split storage,
    rest present but not read" (the existing degree-0 case has degree-0 STORAGE, where there is no rest)."""
    out, ref, model = _fused_raw_parameter_path(gpu_device, 3, active)    # asserts _can_fuse(...) == fused for both runs
    assert model._features_rest.shape[1] == 15 and model.active_sh_degree == active
    for fused in (True, False):
        label = f"render() active degree {active}, fused={fused}"
        img, radii, grads = out[fused]
        _assert_inactive_rows_zero(grads["f_rest"], active, label)
        print(f"[kinds] {label}: {_assert_three_kinds(radii, grads, label)}")
    _assert_inactive_rows_zero(ref["f_rest"], active, "oracle")


# ---- 5. the result does not depend on the inactive coefficients -----------------------------------------------------------
@pytest.fixture()
def fresh_state(monkeypatch):
    """No remembered capacity before or after; GSR_SYNC_FREE's default mode (as test_gpu_sync_free.py)."""
    from mvs_gaussian_splatting_amd import rasterizer
    rasterizer.synchronize_counts()
    rasterizer._states.clear()
    monkeypatch.setattr(rasterizer, "_sync_free_value", rasterizer.SYNC_VERIFIED)
    yield rasterizer
    try:
        rasterizer.synchronize_counts()
    except Exception:
        pass
    rasterizer._states.clear()


def _device_scene(dev, active, overwrite=None, P=2500, stored=3):
    """The backward scene on the device with active_sh_degree = active.  overwrite: "huge" / "nan": every coefficient of a
    degree above the active one becomes +-1e30 (random signs) / NaN."""
    model, cam, _, target = small_scene(P=P, sh_degree=stored, width=208, height=120, scale=0.06)
    model.active_sh_degree = active
    used = _n_rest(active)
    if overwrite == "huge":
        sign = torch.randint(0, 2, model._features_rest[:, used:].shape, generator=torch.Generator().manual_seed(9)) * 2 - 1
        model._features_rest[:, used:] = 1e30 * sign.float()
    elif overwrite == "nan":
        model._features_rest[:, used:] = float("nan")
    else:
        assert overwrite is None
    model.to(dev); cam.to(dev)
    for p in model.parameters():
        p.requires_grad_(True)
    return model, cam, torch.tensor(BG, device=dev), target.to(dev)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "getters"])
@pytest.mark.parametrize("active", [0, 1, 2])
def test_result_does_not_depend_on_the_inactive_coefficients(gpu_device, fresh_state, active, fused):
    """The reference never reads a coefficient above the active degree.  Two frames per model (the first through the
    two-call forward, the second of the same P through the sync-free gsr_forward), as generated and with the inactive
    coefficients overwritten: image, radii and every gradient bit-identical.  NaN catches a `0 * x` where 1e30 may not."""
    from test_gpu_sync_free import _step
    rz = fresh_state
    runs = {}
    for kind in (None, "huge", "nan"):
        rz.synchronize_counts()
        rz._states.clear()
        model, cam, bg, target = _device_scene(gpu_device, active, kind)
        if kind == "nan":
            assert bool(torch.isnan(model._features_rest[:, _n_rest(active):]).all())
            assert bool(torch.isfinite(model._features_rest[:, :_n_rest(active)]).all())
        frames = []
        for f in range(2):
            pkg, g = _step(model, cam, bg, target, fused)
            ctx = pkg["render"].grad_fn
            if f == 0:
                R0, _ = rz.frame_counts(pkg["render"])
                assert ctx.layout[0] == R0 > 1000                              # two-call path: laid out for its own count
            else:
                assert ctx.layout[0] >= int(1.5 * R0) and ctx.layout[1] == 2500   # gsr_forward: laid out for a capacity
            frames.append((pkg["render"].detach().clone(), pkg["radii"].clone(), g))
        assert rz.reissued_frames(gpu_device, 2500, cam.image_width, cam.image_height) == 0
        runs[kind] = frames
    names = ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity", "means2D")
    for f in range(2):
        img0, radii0, g0 = runs[None][f]
        assert bool(torch.isfinite(img0).all()) and int((radii0 > 0).sum()) > 100
        _assert_inactive_rows_zero(g0[2].cpu(), active, f"clean model, frame {f}")
        for kind in ("huge", "nan"):
            img, radii, g = runs[kind][f]
            what = f"inactive coefficients = {kind}, active degree {active}, fused={fused}, frame {f}"
            assert torch.equal(img, img0), f"{what}: the image depends on them"
            assert torch.equal(radii, radii0), f"{what}: the radii depend on them"
            for k, a, b in zip(names, g, g0):
                assert torch.equal(a, b), f"{what}: the gradient of {k} depends on them"
    for a, b in zip(runs[None][0][2], runs[None][1][2]):                   # and the two forwards agree (sync-free parity)
        assert torch.equal(a, b)
    assert torch.equal(runs[None][0][0], runs[None][1][0])


# ---- 6. the degree step inside a run --------------------------------------------------------------------------------------
@pytest.mark.parametrize("lower", [0, 1, 2])
def test_degree_step_inside_a_run_costs_no_readback_and_changes_nothing_else(gpu_device, fresh_state, lower):
    """Iteration 1000 of train.py: frames at degree `lower` until the capacity state exists, then one train step (frame,
    backward with the fused densification statistics, Adam) at lower + 1 issued into that state -- against the same step
    issued into a fresh state, bit for bit, without a re-issued frame."""
    from mvs_gaussian_splatting_amd import render, l1_loss, add_densification_stats
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    rz = fresh_state
    dev = gpu_device
    pipe = PipelineParams()
    pipe.fuse_densify_stats = True
    P = 2500

    def train_step(model, cam, bg, target, opt, forbid_sync=False):
        opt.zero_grad(set_to_none=True)
        for t in (model.xyz_gradient_accum, model.denom, model.max_radii2D):
            t.zero_()
        if forbid_sync:                              # the forward of the step frame reads nothing back through torch
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
        try:
            pkg = render(cam, model, pipe, bg)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        assert pkg["viewspace_points"]._gsr_stats_fused
        l1_loss(pkg["render"], target).backward()
        add_densification_stats(model, pkg["viewspace_points"], pkg["radii"])
        res = {"image": pkg["render"].detach().clone(), "radii": pkg["radii"].clone(),
               "means2D": pkg["viewspace_points"].grad.clone()}
        res.update({"grad" + k: getattr(model, k).grad.clone() for k in model._PARAMS})
        opt.step()
        res.update({"stepped" + k: getattr(model, k).detach().clone() for k in model._PARAMS})
        res.update({k: getattr(model, k).clone() for k in ("xyz_gradient_accum", "denom", "max_radii2D")})
        return pkg, res

    def problem(active):
        model, cam, bg, target = _device_scene(dev, active)
        return model, cam, bg, target, torch.optim.Adam(model.parameters(), lr=1e-3, eps=1e-15)

    # (a) into the state the lower degree left behind
    model, cam, bg, target, opt = problem(lower)
    for f in range(2):
        pkg = render(cam, model, pipe, bg)
        l1_loss(pkg["render"], target).backward()
    lower_image = pkg["render"].detach().clone()
    assert pkg["render"].grad_fn.layout[1] == P and len(rz._states) == 1   # the capacity state exists and is in use
    W, H = cam.image_width, cam.image_height
    before = rz.reissued_frames(dev, P, W, H)
    model.active_sh_degree = lower + 1
    pkg, got = train_step(model, cam, bg, target, opt, forbid_sync=True)    # the first frame at the new degree
    ctx = pkg["render"].grad_fn
    assert ctx.frame_pending is None and ctx.layout[1] == P and ctx.layout[0] >= int(1.5 * ctx.counts[0])
    assert rz.reissued_frames(dev, P, W, H) == before == 0
    assert len(rz._states) == 1
    # (b) the same step into a fresh state
    rz.synchronize_counts()
    rz._states.clear()
    model2, cam2, bg2, target2, opt2 = problem(lower + 1)
    pkg2, want = train_step(model2, cam2, bg2, target2, opt2)
    assert pkg2["render"].grad_fn.layout == rz.frame_counts(pkg2["render"])   # two-call path
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), f"degree {lower} -> {lower + 1}: {k} differs from the fresh-state frame"
    assert not torch.equal(got["image"], lower_image)                      # the step is visible in the image
    if lower + 1 < 3:
        _assert_inactive_rows_zero(got["grad_features_rest"].cpu(), lower + 1, "stepped frame")
    assert float(got["denom"].sum()) == float((got["radii"] > 0).sum()) > 0


# ---- 7. carriers of the degree --------------------------------------------------------------------------------------------
def test_graphed_and_multi_stream_frames_equal_eager_frames_at_degree_1(gpu_device):
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.graphed import GraphedRenderer, MultiStreamRenderer
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from test_gpu_graphed import _cams
    dev = gpu_device
    model, _, _, _ = small_scene(P=6000, sh_degree=3, width=304, height=176, scale=0.03)
    model.to(dev)
    bg = torch.tensor([0.1, 0.3, 0.2], device=dev)
    cams = _cams(dev, 5)
    with torch.no_grad():
        full = [render(cam, model, PipelineParams(), bg)["render"].clone() for cam in cams]
    model.active_sh_degree = 1
    gr = GraphedRenderer(model, PipelineParams(), bg)
    assert gr.fused and gr.sh_degree == 1
    with torch.no_grad():
        for rep in range(2):
            for cam, at3 in zip(cams, full):
                want = render(cam, model, PipelineParams(), bg)
                got = gr.render(cam, verify=(rep == 1))
                assert torch.equal(got["render"], want["render"]) and torch.equal(got["radii"], want["radii"])
                assert torch.equal(got["visibility_filter"], want["visibility_filter"])
                assert not torch.equal(want["render"], at3)                 # degree 1 is not what degree 3 renders
    gr.check()
    assert len(gr.formats) == 1 and next(iter(gr.formats.values())).frames == 10
    mr = MultiStreamRenderer(model, PipelineParams(), bg, streams=2)
    kept = []
    with torch.no_grad():
        for i, out in mr.render_views(cams * 2):
            kept.append(out["render"].clone())
        mr.check()
        assert len(kept) == 2 * len(cams)
        for cam, got in zip(cams * 2, kept):
            assert torch.equal(got, render(cam, model, PipelineParams(), bg)["render"])


@pytest.mark.parametrize("variant", ["grow_dir_distance", "split_both"])
def test_grown_and_learned_split_frame_at_degree_1(gpu_device, variant):
    """One open grow frame and one learned-split frame of test_gpu_grow.py's end-to-end test at active_sh_degree = 1:
    folded gradients against the reference restatement at that test's bars; the folded f_rest gradient of all P source
    rows is an exact zero above degree 1."""
    from test_gpu_grow import _grown_frame_end_to_end
    got, P = _grown_frame_end_to_end(gpu_device, variant, active_sh_degree=1)
    assert got["f_rest"].shape == (P, 15, 3) and P % 64 != 0
    _assert_inactive_rows_zero(got["f_rest"].cpu(), 1, f"{variant} at degree 1")


def test_convert_SHs_python_and_in_kernel_sh_match_the_oracle_at_degree_1(gpu_device):
    """pipe.convert_SHs_python evaluates eval_sh(active_sh_degree, ...) in torch and hands colours to the operator; the
    default evaluates the SH in the preprocess kernel.  Both images against the float64 oracle at degree 1 by the forward
    rule of the suite (robust pixels 1e-5 * max(1, |ref|), any pixel 2/255), the gradients of the convert mode at the
    compare_grads bar."""
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.renderer import _can_fuse
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from grad_util import grads_oracle, compare_grads, masked_l1
    dev = gpu_device
    active = 1
    model, cam, _, target = small_scene(P=2500, sh_degree=3, width=208, height=120, scale=0.06)
    model.active_sh_degree = active
    bg = torch.tensor(BG)
    st_o = make_settings(cam, bg, active)
    ref, weight, aux, col = grads_oracle(model, st_o, target)
    ref32, _, _, _ = grads_oracle(model, st_o, target, dtype=torch.float32, weight=weight)
    robust = aux["margin"] > 1e-4
    n_fragile = int((~robust).sum())
    assert n_fragile <= 0.01 * robust.numel()
    model.to(dev); cam.to(dev)
    for convert in (True, False):
        for p in model.parameters():
            p.grad = None
            p.requires_grad_(True)
        pipe = PipelineParams()
        pipe.convert_SHs_python = convert
        assert _can_fuse(model, pipe, None) == (not convert)
        pkg = render(cam, model, pipe, bg.to(dev))
        masked_l1(pkg["render"], target, weight).backward()
        err = ((pkg["render"].detach().cpu().double() - col).abs() / col.abs().clamp(min=1.0)).max(dim=0).values
        print(f"[pixels] convert_SHs_python={convert}, degree {active}: worst robust pixel {float(err[robust].max()):.2e}, "
              f"worst pixel {float(err.max()):.2e}, fragile pixels {n_fragile}")
        assert float(err[robust].max()) <= 1e-5 and float(err.max()) <= 2.0 / 255.0
        got = {"xyz": model._xyz.grad, "f_dc": model._features_dc.grad, "f_rest": model._features_rest.grad,
               "opacity": model._opacity.grad, "scaling": model._scaling.grad, "rotation": model._rotation.grad,
               "means2D": pkg["viewspace_points"].grad}
        got = {k: v.detach().cpu() for k, v in got.items()}
        compare_grads(got, ref, ref32, f"render() convert_SHs_python={convert}, stored degree 3, active {active} "
                                       f"(fragile pixels {n_fragile})")
        _assert_inactive_rows_zero(got["f_rest"], active, f"convert_SHs_python={convert}")


# ---- 8. a training loop that crosses the steps ----------------------------------------------------------------------------
def test_training_loop_crosses_the_degree_steps(gpu_device):
    """examples/train_synthetic.py with the reference's schedule scaled down (a step every 15 iterations, 60 iterations,
    densification every 20): torch.optim.Adam and the HIP Adam bit-identical; until a band of coefficients becomes active
    nothing has moved it (the example starts f_rest at zero; clone / split copy rows) and its Adam moments are exact
    zeros; afterwards every band has moved; the loss went down."""
    from train_synthetic import train
    from mvs_gaussian_splatting_amd import optim
    from mvs_gaussian_splatting_amd.densify import GROUP_ATTR
    from test_gpu_adam import _assert_same
    runs, steps = {}, {}

    def before_step(kind):
        def check(it, model):
            D = model.active_sh_degree
            used = _n_rest(D)
            rest = model._features_rest
            assert rest.shape[1] == 15 and int(torch.count_nonzero(rest.detach()[:, used:])) == 0, \
                f"{kind}, iteration {it}: coefficients above degree {D} moved before they became active"
            state = model.optimizer.state[rest]
            for key in ("exp_avg", "exp_avg_sq"):
                assert state[key].shape == rest.shape and int(torch.count_nonzero(state[key][:, used:])) == 0, \
                    f"{kind}, iteration {it}: {key} of the coefficients above degree {D} is not zero"
            if used:
                assert int(torch.count_nonzero(rest.detach()[:, :used])) > 0
            steps[kind].append((it, D, rest.shape[0]))
        return check

    for kind in ("torch", "hip"):
        torch.manual_seed(0)
        steps[kind] = []
        runs[kind] = train(gpu_device, iterations=60, densification_interval=20, densify_from_iter=10, optimizer=kind,
                           sh_increase_every=15, on_sh_increase=before_step(kind))
    (ma, ha, sa), (mb, hb, sb) = runs["torch"], runs["hip"]
    assert isinstance(mb.optimizer, optim.Adam)
    assert steps["torch"] == steps["hip"] and [s[:2] for s in steps["hip"]] == [(15, 0), (30, 1), (45, 2)]
    assert steps["hip"][-1][2] > steps["hip"][0][2]                        # densification ran between the steps
    assert ha == hb and sa == sb and len(sa) > 0
    _assert_same(ma, mb, "train_synthetic with degree steps")
    for a in GROUP_ATTR.values():
        assert torch.equal(getattr(ma, a), getattr(mb, a))
    assert mb.active_sh_degree == 3 == mb.max_sh_degree
    for lo, hi in ((0, 3), (3, 8), (8, 15)):
        assert int(torch.count_nonzero(mb._features_rest.detach()[:, lo:hi])) > 0, f"band {lo}:{hi} never moved"
    # 8 views in rotation: a mean over 8 iterations has every view in it once
    first, last = sum(hb[:8]) / 8, sum(hb[-8:]) / 8
    assert all(h == h for h in hb) and last < first, (first, last)
