"""Self-consistency of the CPU oracle (the rasterizer boundary itself is unpinned by the reference, so the
restatement is checked against independent properties).  CPU only, small scenes."""
import math

import numpy as np
import pytest
import torch

from conftest import make_settings, small_scene


def _run(model, cam, bg, deg, dtype=torch.float64, **kw):
    from oracle import rasterize_ref
    c = lambda t: t.to(dtype)  # noqa: E731
    return rasterize_ref(c(model.get_xyz), None, c(model.get_opacity), make_settings(cam, bg, deg),
                         shs=c(model.get_features), scales=c(model.get_scaling), rotations=c(model.get_rotation), **kw)


def test_weights_plus_final_T_sum_to_one():
    """With colour == 1 everywhere and bg == 1 the composite is sum(w_i) + T_final == 1 for every pixel."""
    from oracle import rasterize_ref
    model, cam, _, _ = small_scene(P=600, sh_degree=0, width=96, height=64, focal=40.0)
    ones = torch.ones(600, 3, dtype=torch.float64)
    bg = torch.ones(3)
    col, radii = rasterize_ref(model.get_xyz.double(), None, model.get_opacity.double(), make_settings(cam, bg, 0),
                               colors_precomp=ones, scales=model.get_scaling.double(), rotations=model.get_rotation.double())
    assert int((radii > 0).sum()) > 100
    # pixels that terminated early lose at most T_STOP of mass
    assert float((col - 1.0).abs().max()) < 1.1e-4


def test_zero_opacity_gives_background_and_culls_nothing_visible():
    from oracle import rasterize_ref
    model, cam, _, _ = small_scene(P=300, sh_degree=1, width=64, height=48, focal=30.0)
    bg = torch.tensor([0.2, 0.4, 0.6])
    col, radii = rasterize_ref(model.get_xyz, None, torch.zeros(300, 1), make_settings(cam, bg, 1),
                               shs=model.get_features, scales=model.get_scaling, rotations=model.get_rotation)
    assert torch.allclose(col, bg.view(3, 1, 1).expand_as(col))
    assert int((radii > 0).sum()) > 0


def test_binning_is_sorted_and_ranges_partition_the_list():
    model, cam, bg, _ = small_scene(P=1500, sh_degree=0, width=160, height=96, focal=80.0)
    col, radii, aux = _run(model, cam, bg, 0, dtype=torch.float32, want_aux=True)
    keys, ranges = aux["keys"], aux["ranges"]
    assert np.all(keys[1:] >= keys[:-1])
    nonempty = ranges[:, 1] > ranges[:, 0]
    assert int((ranges[nonempty, 1] - ranges[nonempty, 0]).sum()) == keys.size == int(aux["pre"]["tiles_touched"].sum())
    tile = (keys >> np.uint64(32)).astype(np.int64)
    for t in np.nonzero(nonempty)[0][:50]:
        assert np.all(tile[ranges[t, 0]:ranges[t, 1]] == t)
    # equal (tile, depth) keep Gaussian-index order (stable sort of index-ordered emission)
    same = keys[1:] == keys[:-1]
    assert np.all(aux["point_list"][1:][same] > aux["point_list"][:-1][same])


def test_fp32_and_fp64_runs_agree_on_robust_pixels():
    model, cam, bg, _ = small_scene(P=1500, sh_degree=2, width=128, height=80, focal=64.0)
    c32, r32, a32 = _run(model, cam, bg, 2, dtype=torch.float32, want_aux=True, want_margin=True)
    c64, r64 = _run(model, cam, bg, 2, dtype=torch.float64)
    assert int((r32 != r64).sum()) <= 2
    robust = a32["margin"] > 1e-4
    err = (c32.double() - c64).abs().max(dim=0).values
    assert float(err[robust].max()) < 1e-5   # fp32 rounding of a few hundred blended terms


@pytest.mark.parametrize("use_cov", [False, True])
def test_autograd_matches_finite_differences(use_cov):
    """Gradient truth check: fp64 autograd of the restatement vs central differences of a smooth loss.
    exact_grad (upstream_grad=False) is used because finite differences see the exact derivative; the two
    documented upstream deviations are checked separately below."""
    _autograd_vs_finite_differences(1, 1, use_cov)


def _autograd_vs_finite_differences(stored, active, use_cov):
    """SH storage of degree `stored` evaluated at degree `active`; returns the autograd gradient of f_rest."""
    from oracle import rasterize_ref
    torch.manual_seed(0)
    model, cam, bg, target = small_scene(P=40, sh_degree=stored, width=48, height=32, scale=0.25, focal=40.0)
    bg = torch.tensor([0.1, 0.3, 0.2], dtype=torch.float64)
    st = make_settings(cam, bg, active)
    d = torch.float64
    xyz = model._xyz.to(d).requires_grad_(True)
    op = model._opacity.to(d).requires_grad_(True)
    fdc = model._features_dc.to(d).requires_grad_(True)
    frest = model._features_rest.to(d).requires_grad_(True)
    sc = model._scaling.to(d).requires_grad_(True)
    rot = model._rotation.to(d).requires_grad_(True)
    wgt = torch.rand(3, 32, 48, dtype=d, generator=torch.Generator().manual_seed(2))

    def f():
        kw = {}
        if use_cov:
            from oracle import build_cov3d_ref
            kw["cov3D_precomp"] = build_cov3d_ref(torch.exp(sc), 1.0, torch.nn.functional.normalize(rot))
        else:
            kw["scales"], kw["rotations"] = torch.exp(sc), torch.nn.functional.normalize(rot)
        col, _ = rasterize_ref(xyz, None, torch.sigmoid(op), st, shs=torch.cat((fdc, frest), 1), upstream_grad=False, **kw)
        return (col * wgt).sum()

    loss = f()
    grads = torch.autograd.grad(loss, [xyz, op, fdc, frest, sc, rot])
    rng = np.random.default_rng(0)
    eps = 1e-6
    for p, g in zip([xyz, op, fdc, frest, sc, rot], grads):
        flat = p.detach().view(-1)
        for idx in rng.choice(flat.numel(), size=6, replace=False):
            old = flat[idx].item()
            with torch.no_grad():
                flat[idx] = old + eps
                lp = f().item()
                flat[idx] = old - eps
                lm = f().item()
                flat[idx] = old
            fd = (lp - lm) / (2 * eps)
            an = g.reshape(-1)[idx].item()
            assert abs(fd - an) <= 2e-4 * max(1.0, abs(an)) + 2e-6, (p.shape, idx, fd, an)
    return grads[3]


@pytest.mark.parametrize("stored,active", [(3, 1), (2, 0)])
def test_autograd_matches_finite_differences_below_the_stored_sh_degree(stored, active):
    """The oracle is the truth for the GPU tests that render a model at an active SH degree below the one its storage was
    sized for (every training run's first 3000 iterations): same scene size, step and bar as above, and the gradient of
    the coefficients above the active degree is not small but exactly zero."""
    g_rest = _autograd_vs_finite_differences(stored, active, False)
    used = (active + 1) ** 2 - 1
    assert g_rest.shape[1] == (stored + 1) ** 2 - 1 > used
    assert int(torch.count_nonzero(g_rest[:, used:])) == 0
    if used:
        assert int(torch.count_nonzero(g_rest[:, :used])) > 0


@pytest.mark.parametrize("stored,active", [(3, 0), (3, 1), (3, 2), (2, 1), (1, 0)])
def test_image_below_the_stored_sh_degree_is_the_image_of_the_truncated_model(stored, active):
    """Degree `active` of a degree-`stored` model reads the first (active + 1)^2 coefficients and nothing else: the image
    and the radii equal those of the model cut down to degree-`active` storage, bit for bit in float64 -- also when the
    coefficients above are not finite."""
    from oracle import rasterize_ref
    model, cam, _, _ = small_scene(P=1200, sh_degree=stored, width=112, height=80, focal=60.0, scale=0.07)
    bg = torch.tensor([0.2, 0.3, 0.1])
    used = (active + 1) ** 2
    d = torch.float64
    kw = dict(scales=model.get_scaling.to(d), rotations=model.get_rotation.to(d))
    shs = model.get_features.to(d)
    st = make_settings(cam, bg, active)
    full = rasterize_ref(model.get_xyz.to(d), None, model.get_opacity.to(d), st, shs=shs, **kw)
    cut = rasterize_ref(model.get_xyz.to(d), None, model.get_opacity.to(d), st, shs=shs[:, :used].contiguous(), **kw)
    poisoned = shs.clone()
    poisoned[:, used:] = float("nan")
    nan = rasterize_ref(model.get_xyz.to(d), None, model.get_opacity.to(d), st, shs=poisoned, **kw)
    assert int((full[1] > 0).sum()) > 100
    for other in (cut, nan):
        assert torch.equal(full[0], other[0]) and torch.equal(full[1], other[1])
    higher = rasterize_ref(model.get_xyz.to(d), None, model.get_opacity.to(d), make_settings(cam, bg, stored), shs=shs, **kw)
    assert not torch.equal(full[0], higher[0])          # ... and the degree really changes the image


def test_upstream_gradient_deviations_are_small_and_documented():
    """upstream_grad=True differs from the exact derivative only through (a) the 1/(det^2 + 1e-7) conic
    denominator, (b) the unclamped alpha gradient, (c) the zeroed guard-band path."""
    from oracle import rasterize_ref
    model, cam, bg, target = small_scene(P=300, sh_degree=0, width=64, height=48, scale=0.08, focal=30.0)
    d = torch.float64
    res = []
    for up in (True, False):
        xyz = model._xyz.to(d).requires_grad_(True)
        sc = model._scaling.to(d).requires_grad_(True)
        col, _ = rasterize_ref(xyz, None, model.get_opacity.to(d) * 0.5, make_settings(cam, bg, 0),
                               shs=model.get_features.to(d), scales=torch.exp(sc),
                               rotations=model.get_rotation.to(d), upstream_grad=up)
        (col - target.to(d)).abs().mean().backward()
        res.append((xyz.grad.clone(), sc.grad.clone()))
    for a, b in zip(res[0], res[1]):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())


@pytest.mark.parametrize("deg,use_cov", [(3, False), (1, False), (0, True)])
def test_c_oracle_agrees_with_pytorch_oracle(deg, use_cov):
    """Two independent CPU restatements (scalar C loops in upstream's per-pixel order vs vectorised PyTorch):
    integers identical, pixels equal on every robust pixel."""
    from oracle import rasterize_ref
    from oracle.c_oracle import forward_c
    model, cam, _, _ = small_scene(P=1200, sh_degree=deg, width=112, height=80, focal=60.0, scale=0.07)
    bg = torch.tensor([0.2, 0.3, 0.1])
    st = make_settings(cam, bg, deg)
    kw = dict(shs=model.get_features)
    if use_cov:
        kw["cov3D_precomp"] = model.get_covariance(1.0)
    else:
        kw["scales"], kw["rotations"] = model.get_scaling, model.get_rotation
    col, radii, aux = rasterize_ref(model.get_xyz, None, model.get_opacity, st, want_aux=True, want_margin=True, **kw)
    c = forward_c(model.get_xyz, model.get_opacity, st, **kw)
    assert np.array_equal(c["radii"], radii.numpy())
    assert c["R"] == aux["keys"].size and np.array_equal(c["keys"], aux["keys"])
    assert np.array_equal(c["point_list"], aux["point_list"]) and np.array_equal(c["ranges"], aux["ranges"])
    robust = (aux["margin"] > 1e-4).numpy()
    err = np.abs(c["color"] - col.numpy()).max(axis=0)
    assert err[robust].max() <= 2e-6
    assert np.array_equal(c["n_contrib"][robust], aux["n_contrib"].numpy().astype(np.uint32)[robust])
    assert np.abs(c["final_T"] - aux["final_T"].numpy())[robust].max() <= 1e-6


def test_densify_restatement_invariants():
    """oracle/densify_ref.py: row order, counts, statistics reset, moment surgery, children geometry."""
    import math
    from oracle.densify_ref import densify_and_prune_ref, count_split_selected_ref, GROUPS
    g = torch.Generator().manual_seed(0)
    P = 4000
    params = {"xyz": torch.randn(P, 3, generator=g), "f_dc": torch.randn(P, 1, 3, generator=g),
              "f_rest": torch.randn(P, 15, 3, generator=g), "opacity": 2.5 * torch.randn(P, 1, generator=g) - 1.0,
              "scaling": math.log(0.05) + 1.2 * torch.randn(P, 3, generator=g), "rotation": torch.randn(P, 4, generator=g)}
    moments = {k: (torch.randn(v.shape, generator=g), torch.rand(v.shape, generator=g)) for k, v in params.items()}
    denom = torch.randint(0, 4, (P, 1), generator=g).float()
    accum = torch.rand(P, 1, generator=g) * 0.0006 * denom
    radii = torch.rand(P, generator=g) * 40
    extent, pd, thr, min_op = 5.0, 0.01, 0.0002, 0.005
    n_sel = count_split_selected_ref(params, accum.clone(), denom, pd, thr, extent)
    noise = torch.randn(2 * n_sel, 3, generator=g)
    p, m, a, d, r, info = densify_and_prune_ref(params, moments, accum, denom, radii, pd, thr, min_op, extent, 20, noise)
    n = p["xyz"].shape[0]
    assert info["split"] == n_sel and n == P + info["cloned"] + info["split"] - info["pruned"]
    assert all(p[k].shape[0] == n and m[k][0].shape == p[k].shape for k in GROUPS)
    assert a.shape == (n, 1) and float(a.abs().max()) == 0 and float(d.abs().max()) == 0 and float(r.abs().max()) == 0
    # survivors respect the prune rules; no split parent survives as-is (its scale would exceed its children's)
    assert float(torch.sigmoid(p["opacity"]).min()) >= min_op and float(torch.exp(p["scaling"]).max()) <= 0.1 * extent
    # kept originals come first, in order, with their moments; appended rows have zero moments
    grads = accum / denom
    grads[grads.isnan()] = 0
    sc = torch.exp(params["scaling"]).max(dim=1).values
    split = (grads.squeeze(-1) >= thr) & (sc > pd * extent)
    prune = (torch.sigmoid(params["opacity"]).squeeze(-1) < min_op) | (sc > 0.1 * extent)
    keep = ~split & ~prune
    nk = int(keep.sum())
    assert torch.equal(p["xyz"][:nk], params["xyz"][keep]) and torch.equal(m["f_rest"][0][:nk], moments["f_rest"][0][keep])
    assert float(m["xyz"][0][nk:].abs().max()) == 0 and float(m["xyz"][1][nk:].abs().max()) == 0
    # max_screen_size None: only the opacity rule prunes
    p2 = densify_and_prune_ref(params, None, accum, denom, radii, pd, thr, min_op, extent, None, noise)[0]
    assert p2["xyz"].shape[0] >= n and float(torch.exp(p2["scaling"]).max()) > 0.1 * extent


def test_c_oracle_is_clean_under_asan_and_ubsan():
    """SURVEY §5 (sanitizers): the plain-C restatement runs its rare-branch driver (oracle/c/sanitize_main.c) under
    AddressSanitizer + UndefinedBehaviorSanitizer with leaks on, and reproduces the plain build's checksum."""
    import os
    import subprocess
    cdir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "c")
    r = subprocess.run(["make", "-C", cdir, "asan"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "asan/ubsan clean" in r.stdout


# ---- the comparison rules of tests/grad_util.py themselves, with the float32 oracle standing in for a product ---------------
def test_all_pixel_rules_hold_for_an_independent_float32_implementation():
    """The all-pixel run of the GPU parity tests (grad_util: discontinuity-free loss over EVERY pixel; strict bar without
    threshold-fragile pixels, per-scene bar with them) must at least accept the float32 oracle -- an implementation that
    shares nothing with the HIP kernels -- and must reject a gradient that is off by a percent."""
    import pytest
    from conftest import small_scene, make_settings
    from grad_util import (grads_oracle, compare_grads, compare_grads_unmasked, linear_weights)
    seen = set()
    for seed in (0, 2):
        model, cam, _, target = small_scene(P=1200, sh_degree=1, width=112, height=80, scale=0.06, seed=seed)
        bg = torch.tensor([0.3, 0.1, 0.2])
        st = make_settings(cam, bg, 1)
        _, weight, aux, _ = grads_oracle(model, st, target)
        n_fragile = int((aux["margin"] <= 1e-4).sum())
        wts = linear_weights(weight.shape)
        assert float(wts.abs().min()) > 0.0 and wts.shape == weight.shape
        kw = dict(loss_kind="linear")
        ref_u, _, _, _ = grads_oracle(model, st, target, weight=wts, **kw)
        got_u, _, _, _ = grads_oracle(model, st, target, dtype=torch.float32, weight=wts, **kw)
        if n_fragile == 0:
            seen.add("strict")
            compare_grads(got_u, ref_u, got_u, f"seed {seed}")
            bad = {k: (v * 1.01 if k == "xyz" else v) for k, v in got_u.items()}
            with pytest.raises(AssertionError):
                compare_grads(bad, ref_u, got_u, f"seed {seed}, xyz off by 1 %")
        else:
            seen.add("fragile")
            robust_w = wts * (aux["margin"] > 1e-4)[None].to(wts.dtype)
            ref_r, _, _, _ = grads_oracle(model, st, target, weight=robust_w, **kw)
            ref_r32, _, _, _ = grads_oracle(model, st, target, dtype=torch.float32, weight=robust_w, **kw)
            compare_grads_unmasked(got_u, ref_u, n_fragile, f"seed {seed}", ref_masked=ref_r, ref_masked32=ref_r32)
            compare_grads(ref_r32, ref_r, ref_r32, f"seed {seed}, robust pixels only")
            bad = {k: (v * 1.5 if k == "opacity" else v) for k, v in got_u.items()}
            with pytest.raises(AssertionError):
                compare_grads_unmasked(bad, ref_u, n_fragile, f"seed {seed}, opacity off by half", ref_masked=ref_r,
                                       ref_masked32=ref_r32)
    assert seen, "no scene ran"


def test_tiles_are_ranked_by_the_oracle_alone():
    """grad_util.pick_well_conditioned_tiles: the picked tiles are the candidates with the smallest float32-vs-float64
    disagreement of the compositing gradients; the worst picked score is no larger than the worst of all."""
    from conftest import small_scene, make_settings
    from grad_util import pick_well_conditioned_tiles, tile_conditioning
    model, cam, bg, target = small_scene(P=2000, sh_degree=1, width=160, height=96, view=1)
    st = make_settings(cam, bg, 1)
    gx, gy = 10, 6
    cands = [ty * gx + tx for ty in range(0, gy, 2) for tx in range(0, gx, 2)]
    tiles, info = pick_well_conditioned_tiles(model, st, target, cands, 6)
    assert len(tiles) == 6 and set(tiles) <= set(cands) and tiles == sorted(tiles)
    assert info["scores_picked_max"] <= info["scores_all_max"] and info["n_candidates"] == len(cands)
    score, frag = tile_conditioning(model, st, target, cands)
    assert len(score) == len(cands) == len(frag) and min(score) >= 0.0
    best = sorted(range(len(cands)), key=lambda i: (score[i], frag[i]))[:6]
    assert sorted(cands[i] for i in best) == tiles


def test_oracle_on_the_gaussians_of_the_masked_tiles_equals_the_oracle_on_the_whole_model():
    """The full-size GPU tests differentiate the oracle only over the Gaussians that are in the list of a masked tile
    (grad_util.SubModel / members_of_tiles / expand_grads).  On a small scene, against the oracle run on every Gaussian:
    same image in the masked tiles, same weights, same gradients (zero for every Gaussian outside the subset)."""
    from grad_util import grads_oracle, full_frame_lists, members_of_tiles, SubModel, expand_grads
    model, cam, _, target = small_scene(P=2500, sh_degree=2, width=160, height=112, scale=0.05, view=1)
    bg = torch.tensor([0.2, 0.3, 0.1])
    st = make_settings(cam, bg, 2)
    gx = 10
    tiles = [1 * gx + 2, 3 * gx + 7, 5 * gx + 4, 6 * gx + 9]
    mask = torch.zeros(1, 112, 160)
    for t in tiles:
        ty, tx = divmod(t, gx)
        mask[:, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = 1.0
    ref, weight, aux, col = grads_oracle(model, st, target, tiles=tiles, tile_mask=mask)
    lists = full_frame_lists(model, st)
    assert torch.equal(lists[torch.float64][0], aux["radii"])
    idx = members_of_tiles(lists, tiles)
    assert 0 < idx.numel() < 2500
    sub = SubModel(model, idx)
    ref_s, weight_s, aux_s, col_s = grads_oracle(sub, st, target, tiles=tiles, tile_mask=mask)
    assert torch.equal(weight, weight_s) and torch.equal(aux["margin"], aux_s["margin"])
    assert torch.allclose(col, col_s, rtol=0, atol=1e-14)
    full = expand_grads(ref_s, idx, 2500)
    outside = torch.ones(2500, dtype=torch.bool)
    outside[idx] = False
    for k, r in ref.items():
        assert not r[outside].any(), k                   # the whole-model oracle agrees: nothing outside the subset
        assert torch.allclose(full[k], r, rtol=1e-12, atol=1e-18), k
