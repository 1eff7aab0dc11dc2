"""Multi-view depth consistency and back-projection on the HIP path (csrc/mvs.hip, ABI v34; mvs.py)
against the float64 restatement of tests/mvs_restate.py.

Scene: the analytic plane and sphere of ``mvs_restate.scene``: a 70 x 37 reference (past one 64-lane row, ragged on both
axes) and four table rows -- a 48 x 40 source with its own focal lengths, one with a hole of zeros, one scaled by 1.02 in
one half, one facing away.  Bars: ``count`` exactly on the pixels none of whose float64 comparisons is within
``mvs_restate.MARGIN`` of flipping (tests/test_mvs_host.py caps their share at 1 %); ``fused`` max-norm relative to the
pixel's depth within max(1e-5, 2 x the float32 restatement's own error against float64); points likewise relative to
the scene's extent.  The dyadic case of ``mvs_restate.exact_case`` is exact in float32 and is compared on every pixel.
The observed figures are printed (-s).
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from conftest import small_scene
import mvs_restate as R

pytestmark = pytest.mark.gpu


def _bar(ref32, ref64, scale=1.0):
    return max(1e-5, 2.0 * float((np.abs(np.asarray(ref32, np.float64) - ref64) / scale).max()))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _scene():
    ref, depth, cams, depths = R.scene()
    return ref, depth, cams, depths, R.source_rows(ref, cams, depths), R.focal(ref)


@functools.lru_cache(maxsize=None)
def _reference(min_views, order=(0, 1, 2, 3)):
    """float64 and float32 restatement over the table rows ``order``; computed once, never modified."""
    _, depth, _, _, rows, (fx, fy) = _scene()
    rows = [rows[i] for i in order]
    return (R.consistency(depth, fx, fy, rows, R.PIX_THRESH, R.DEPTH_THRESH, min_views),
            R.consistency(depth, fx, fy, rows, R.PIX_THRESH, R.DEPTH_THRESH, min_views, np.float32))


def _table(rows, dev):
    """The device table of the restatement's rows -> (table tensor or None, the tensors it points into)."""
    if not rows:
        return None, []
    from mvs_gaussian_splatting_amd import _lib
    table = (_lib.GsrMvsSource * len(rows))()
    maps = {}
    for k, row in enumerate(rows):
        key = id(row["depth"])
        if key not in maps:
            maps[key] = torch.from_numpy(row["depth"]).to(dev).contiguous()
        t = table[k]
        t.depth, t.width, t.height, t.fx, t.fy = maps[key].data_ptr(), row["W"], row["H"], float(row["fx"]), float(row["fy"])
        for i in range(16):
            t.ref_to_src[i], t.src_to_ref[i] = float(row["A"].reshape(-1)[i]), float(row["B"].reshape(-1)[i])
    return torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev), list(maps.values())


def _raw(dev, depth, fx, fy, rows, min_views, pix=R.PIX_THRESH, dep=R.DEPTH_THRESH):
    """One raw call into outputs pre-filled with garbage -> (count, fused) on the device."""
    from mvs_gaussian_splatting_amd import _lib
    H, W = depth.shape
    d = torch.from_numpy(depth).to(dev)
    table, keep = _table(rows, dev)
    count = torch.full((H, W), 0xAB, dtype=torch.uint8, device=dev)
    fused = torch.full((H, W), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().gsr_mvs_consistency(d.data_ptr(), H, W, float(fx), float(fy),
                                             None if table is None else table.data_ptr(), len(rows), pix, dep, min_views,
                                             count.data_ptr(), fused.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0, _lib.load().gsr_last_error()
        torch.cuda.synchronize()
    del keep
    return count, fused


def _check(tag, count, fused, ref64, ref32, depth, S, scale=1):
    (n, f64, fragile, _), (_, f32, _, _) = ref64, ref32
    has = depth > 0
    ok = has & ~fragile
    got_n, got_f = count.cpu().numpy(), fused.cpu().numpy()
    assert not np.isnan(got_f).any() and got_n.max() <= S, "an output pixel was not written"
    assert np.array_equal(got_n[ok], scale * n[ok]), f"{tag}: counts differ on robust pixels"
    assert np.all(got_n[~has] == 0) and np.all(got_f[~has] == 0), "a pixel without depth gives 0, 0"
    err = float((np.abs(got_f.astype(np.float64) - f64)[ok] / depth[ok]).max())
    bar = _bar(f32[ok], f64[ok], depth[ok])
    print(f"[mvs] {tag}: fused max error {err:.2e} of d (bar {bar:.2e}), {int(ok.sum())} robust pixels, "
          f"{int((has & fragile).sum())} left out, counts {np.bincount(got_n[ok], minlength=4)[:4]}")
    assert err <= bar, f"{tag}: {err:.3e} > {bar:.3e}"
    return got_n, got_f


@pytest.mark.parametrize("min_views", [0, 1, 2, 4])
def test_consistency_matches_the_float64_restatement(gpu_device, min_views):
    _, depth, _, _, rows, (fx, fy) = _scene()
    ref64, ref32 = _reference(min_views)
    count, fused = _raw(gpu_device, depth, fx, fy, rows, min_views)
    got_n, got_f = _check(f"min_views={min_views}", count, fused, ref64, ref32, depth, 4)
    has = depth > 0
    assert np.array_equal(got_f > 0, has & (got_n >= min_views))
    if min_views == 0:
        assert np.all(got_f[has] > 0)
    if min_views == 4:
        assert got_n.max() == 3 and not got_f.any(), "more views asked than sources that see anything: all zeros"
    again_n, again_f = _raw(gpu_device, depth, fx, fy, rows, min_views)
    assert torch.equal(again_n, count) and _same_bits(again_f, fused), "results differ from run to run"


def test_no_source_one_source_and_sixty_four(gpu_device):
    _, depth, _, _, rows, (fx, fy) = _scene()
    d = torch.from_numpy(depth).to(gpu_device)
    count, fused = _raw(gpu_device, depth, fx, fy, [], 0)
    assert not count.any() and _same_bits(fused, d), "S = 0, min_views = 0: fused is the depth"
    count, fused = _raw(gpu_device, depth, fx, fy, [], 1)
    assert not count.any() and not fused.any()
    for k in range(4):
        ref64, ref32 = _reference(1, (k,))
        got_n, _ = _check(f"S=1, row {k}", *_raw(gpu_device, depth, fx, fy, [rows[k]], 1), ref64, ref32, depth, 1)
        assert (k == 3) == (not got_n.any()), "only the camera facing away agrees with nothing"
    ref64, ref32 = _reference(2, tuple(range(4)) * 16)
    base = _reference(2)[0]
    ok = (depth > 0) & ~base[2]
    assert np.array_equal(ref64[0][ok], 16 * base[0][ok])
    got_n, _ = _check("S=64", *_raw(gpu_device, depth, fx, fy, rows * 16, 2), ref64, ref32, depth, 64)
    assert got_n.max() == 48


def test_reordering_the_sources_leaves_the_count_unchanged(gpu_device):
    _, depth, _, _, rows, (fx, fy) = _scene()
    count, fused = _raw(gpu_device, depth, fx, fy, rows, 2)
    for order in ((3, 2, 1, 0), (1, 3, 0, 2)):
        c2, f2 = _raw(gpu_device, depth, fx, fy, [rows[i] for i in order], 2)
        assert torch.equal(c2, count), "every source decides on its own"
        _check(f"order {order}", c2, f2, *_reference(2, order), depth, 4)


def test_dyadic_case_is_exact_on_every_pixel(gpu_device):
    ref, depth, cams, depths = R.exact_case()
    rows, (fx, fy) = R.source_rows(ref, cams, depths), R.focal(ref)
    n, fused, _, _ = R.consistency(depth, fx, fy, rows, 1.0, 0.01, 1)
    count, got = _raw(gpu_device, depth, fx, fy, rows, 1, 1.0, 0.01)
    assert np.array_equal(count.cpu().numpy(), n) and np.array_equal(got.cpu().numpy(), fused.astype(np.float32))
    assert not count[:, 69].any() and bool((count[:, :69] == 1).all()), "us = W_s - 1 exactly has no footprint"
    assert bool((got[:, :69] == 4.0).all())


def test_depth_consistency_wrapper_equals_the_raw_call(gpu_device):
    from mvs_gaussian_splatting_amd import depth_consistency
    ref, depth, cams, depths, rows, (fx, fy) = _scene()
    d = torch.from_numpy(depth).to(gpu_device)
    sd = [torch.from_numpy(m).to(gpu_device) for m in depths]
    for min_views, order in ((2, (0, 1, 2, 3)), (1, (2, 0))):
        count, fused = _raw(gpu_device, depth, fx, fy, [rows[i] for i in order], min_views)
        c2, f2 = depth_consistency(d[None] if min_views == 1 else d, ref, [sd[i] for i in order], [cams[i] for i in order],
                                   pix_thresh=R.PIX_THRESH, depth_thresh=R.DEPTH_THRESH, min_views=min_views)
        assert c2.dtype == torch.uint8 and f2.dtype == torch.float32 and tuple(c2.shape) == tuple(f2.shape) == (37, 70)
        assert torch.equal(c2, count) and _same_bits(f2, fused)
    c0, f0 = depth_consistency(d, ref, [], [], min_views=0)
    assert not c0.any() and _same_bits(f0, d)


# ---- back-projection ---------------------------------------------------------------------------------------------------
def _backproject_raw(dev, depth, fx, fy, c2w, rows_allocated):
    from mvs_gaussian_splatting_amd import _lib
    H, W = depth.shape
    d = torch.from_numpy(depth).to(dev) if depth.size else torch.zeros(1, device=dev)
    xyz = torch.full((rows_allocated, 3), float("nan"), dtype=torch.float32, device=dev)
    m = (C.c_float * 16)(*[float(v) for v in np.asarray(c2w, np.float32).reshape(-1)])
    with torch.cuda.device(dev):
        rc = _lib.load().gsr_depth_backproject(d.data_ptr(), H, W, float(fx), float(fy), C.addressof(m), xyz.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0, _lib.load().gsr_last_error()
        torch.cuda.synchronize()
    return xyz.cpu().numpy()


@pytest.mark.parametrize("shape", [(0, 7), (1, 1), (5, 13), (37, 70)])
def test_backproject_matches_the_restatement(gpu_device, shape):
    H, W = shape
    ref, scene_depth, cams, _, _, _ = _scene()
    pose = cams[0]                                                         # a pose with every matrix entry in play
    cam = R.Cam(np.eye(3), np.zeros(3), max(W, 1), max(H, 1), 40.0, 44.0)
    cam.world_view_transform = pose.world_view_transform
    (fx, fy), c2w = R.focal(cam), R.cam_to_world32(cam)
    if shape == (37, 70):
        depth = scene_depth
    else:
        depth = np.random.default_rng(4).uniform(2.0, 6.0, (H, W)).astype(np.float32)
        depth[depth < 3.0] = 0.0
        if depth.size == 1:
            depth[...] = 3.5
    n = H * W
    got = _backproject_raw(gpu_device, depth, fx, fy, c2w, n + 3)
    assert np.isnan(got[n:]).all(), "a row at or beyond n was written"
    if n == 0:
        return
    ref64, ref32 = R.backproject(depth, fx, fy, c2w), R.backproject(depth, fx, fy, c2w, np.float32)
    has = depth.reshape(-1) > 0
    assert not got[:n][~has].any() and (n < 60 or int((~has).sum()) >= 10), "zero rows where there is no depth"
    extent = float(np.abs(ref64).max())
    err, bar = float(np.abs(got[:n] - ref64).max()) / extent, _bar(ref32, ref64, extent)
    print(f"[mvs] backproject {W} x {H}: max error {err:.2e} of the extent {extent:.2f} (bar {bar:.2e})")
    assert err <= bar
    # through the view matrix again, every point comes back to its pixel
    V = R.view64(cam)

    def reproject(xyz):
        p = xyz[has].astype(np.float64) @ V[:3, :3] + V[3, :3]
        return np.stack((float(fx) * p[:, 0] / p[:, 2] + (W - 1) / 2, float(fy) * p[:, 1] / p[:, 2] + (H - 1) / 2), axis=1)
    py, px = np.nonzero(depth > 0)
    pix = np.stack((px, py), axis=1).astype(np.float64)
    size = float(max(W, H))
    back_err = float(np.abs(reproject(got[:n]) - pix).max()) / size
    back_bar = max(1e-5, 2.0 * float(np.abs(reproject(ref32) - pix).max()) / size)
    print(f"[mvs] re-projected: max error {back_err * size:.2e} pixels (bar {back_bar * size:.2e})")
    assert back_err <= back_bar


# ---- fuse_views and the fused cloud with a stub renderer -----------------------------------------------------------------
def _views(dev):
    """The reference and the three sources that face the scene, as four views with their (doctored) maps on ``dev``."""
    ref, depth, cams, depths, _, _ = _scene()
    views = [R.Cam(np.eye(3), np.zeros(3), 1, 1, 1.0, 1.0) for _ in range(4)]
    for v, c in zip(views, [ref] + cams[:3]):
        v.__dict__.update(c.__dict__)
        v.world_view_transform = c.world_view_transform.to(dev)
    maps = [torch.from_numpy(m).to(dev) for m in [depth] + depths[:3]]
    return views, maps


def _stub_renderer(views, maps):
    """``render`` for the analytic maps: alpha 1 where there is depth (so depth / alpha is the map), a colour from the pixel."""
    calls = []

    def renderer(camera, model, pipe, bg, **kw):
        calls.append(kw)
        d = maps[[id(v) for v in views].index(id(camera))]
        H, W = d.shape
        alpha = (d > 0).to(torch.float32)[None]
        ys, xs = torch.meshgrid(torch.arange(H, device=d.device), torch.arange(W, device=d.device), indexing="ij")
        color = torch.stack((xs / W, ys / H, 0.25 * alpha[0])).to(torch.float32)
        return {"depth": d[None] * alpha, "alpha": alpha, "render": color}
    return renderer, calls


@pytest.mark.parametrize("contracted", [False, True])
def test_fuse_views_with_consistency_equals_the_hand_filled_volume_and_none_is_unchanged(gpu_device, contracted):
    from mvs_gaussian_splatting_amd import (ContractedTSDFVolume, TSDFVolume, depth_consistency, fuse_views,
                                            select_source_views)
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    dev = gpu_device
    model, _, bg, _ = small_scene(P=16)
    model.to(dev)
    bg, pipe = bg.to(dev), PipelineParams()
    views, maps = _views(dev)
    renderer, calls = _stub_renderer(views, maps)
    if contracted:
        make = lambda: ContractedTSDFVolume((-1.5,) * 3, 3.0 / 40, (41, 41, 41), 0.25, (0.0, 0.0, 3.0), 1.0, device=dev)   # noqa: E731
    else:
        make = lambda: TSDFVolume((-1.75, -1.0, 2.5), 0.05, (70, 40, 40), 0.2, device=dev)      # noqa: E731
    options = dict(n_sources=3, min_views=2, pix_thresh=R.PIX_THRESH, depth_thresh=R.DEPTH_THRESH, max_angle_deg=75.0)
    filtered = fuse_views(views, model, pipe, bg, make(), renderer=renderer, consistency=options)
    assert calls == [{"return_depth": True}] * 4, "every view is rendered once"
    plain = fuse_views(views, model, pipe, bg, make(), renderer=renderer)
    defaults = fuse_views(views, model, pipe, bg, make(), renderer=renderer, consistency={})
    by_hand, by_hand_plain = make(), make()
    sources = select_source_views(views, 3, 75.0)
    assert all(len(s) == 3 for s in sources)
    dropped = 0
    for i, (cam, d) in enumerate(zip(views, maps)):
        color = renderer(cam, model, pipe, bg)["render"]
        by_hand_plain.integrate(d[None], cam, color=color)
        count, _ = depth_consistency(d, cam, [maps[j] for j in sources[i]], [views[j] for j in sources[i]],
                                     pix_thresh=R.PIX_THRESH, depth_thresh=R.DEPTH_THRESH, min_views=2)
        kept = torch.where(count >= 2, d, torch.zeros_like(d))
        dropped += int(((d > 0) & (kept == 0)).sum())
        by_hand.integrate(kept[None], cam, color=color)
    updated, updated_plain = int((filtered.weight > 0).sum()), int((plain.weight > 0).sum())
    print(f"[mvs] fuse_views contracted={contracted}: {updated} points updated with the filter, {updated_plain} without; "
          f"{dropped} pixels dropped")
    assert dropped > 1000 and 500 < updated < updated_plain
    for name in ("tsdf", "weight", "color"):
        assert _same_bits(getattr(filtered, name), getattr(by_hand, name)), name
        assert _same_bits(getattr(plain, name), getattr(by_hand_plain, name)), f"{name} with consistency=None"
    assert not _same_bits(filtered.weight, plain.weight)
    assert int((defaults.weight > 0).sum()) > 0


def _surface_distance(p):
    plane = np.abs(p @ R.PLANE_N - R.PLANE_C) / np.linalg.norm(R.PLANE_N)
    return np.minimum(plane, np.abs(np.linalg.norm(p - R.SPHERE_O, axis=1) - R.SPHERE_R))


def test_fuse_depth_points_gathers_the_consistent_pixels_in_view_then_pixel_order_on_the_surfaces(gpu_device):
    from mvs_gaussian_splatting_amd import (backproject_depth, depth_consistency, evaluate_points, fuse_depth_points,
                                            select_source_views)
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    dev = gpu_device
    model, _, bg, _ = small_scene(P=16)
    bg, pipe = bg.to(dev), PipelineParams()
    views, maps = _views(dev)
    renderer, calls = _stub_renderer(views, maps)
    xyz, rgb = fuse_depth_points(views, model, pipe, bg, n_sources=3, min_views=2, pix_thresh=R.PIX_THRESH,
                                 depth_thresh=R.DEPTH_THRESH, max_angle_deg=75.0, renderer=renderer)
    assert calls == [{"return_depth": True}] * 4
    assert xyz.dtype == rgb.dtype == torch.float32 and xyz.shape == rgb.shape and xyz.shape[1] == 3
    sources = select_source_views(views, 3, 75.0)
    want_xyz, want_rgb, own, ranges, doctored = [], [], [], [], 0
    half = torch.zeros_like(maps[3], dtype=torch.bool)
    half[:, :34] = True                                                    # the 1.02 half of the last view
    for i, (cam, d) in enumerate(zip(views, maps)):
        _, fused = depth_consistency(d, cam, [maps[j] for j in sources[i]], [views[j] for j in sources[i]],
                                     pix_thresh=R.PIX_THRESH, depth_thresh=R.DEPTH_THRESH, min_views=2)
        valid = (fused > 0).reshape(-1)
        if i == 3:
            doctored = int((valid & half.reshape(-1)).sum())
        pts = backproject_depth(fused, cam)
        assert not pts[~valid].any()
        want_xyz.append(pts[valid])
        want_rgb.append(renderer(cam, model, pipe, bg)["render"].reshape(3, -1).t()[valid])
        # the same pixels at the view's own depth, and their distance from the camera
        own.append(backproject_depth(d, cam)[valid].cpu().numpy().astype(np.float64))
        ranges.append(np.linalg.norm(own[-1] - np.linalg.inv(R.view64(cam))[3, :3], axis=1))
    per_view = [int(w.shape[0]) for w in want_xyz]
    assert xyz.shape[0] == sum(per_view) and min(per_view) > 100
    assert _same_bits(xyz, torch.cat(want_xyz)) and _same_bits(rgb, torch.cat(want_rgb)), "view order, then pixel order"
    assert doctored == 0, "the half scaled by 1.02 contributes no point"
    # a view's own depth lies on a surface unless it was doctored (the 1.014 patch survives in places: 1.4 % is below
    # what its neighbours can see); a consistent round trip lies within depth_thresh * d of d along the pixel's ray, so
    # the fused point lies within depth_thresh times its range of the pixel's own point
    p, own, ranges = xyz.cpu().numpy().astype(np.float64), np.concatenate(own), np.concatenate(ranges)
    extent = float(np.abs(own).max())
    on_surface = _surface_distance(own) <= 1e-5 * extent
    off = _surface_distance(p)
    print(f"[mvs] fused cloud: {per_view} points per view, {int((~on_surface).sum())} from doctored pixels; largest distance "
          f"from the surfaces {off[on_surface].max():.2e}, largest share of depth_thresh * range "
          f"{(off[on_surface] / (R.DEPTH_THRESH * ranges[on_surface])).max():.3f}")
    assert int(on_surface.sum()) > 0.9 * len(p)
    assert np.all(off[on_surface] <= R.DEPTH_THRESH * ranges[on_surface] + 1e-5 * extent)
    # against points sampled from the analytic surfaces: the accuracy stays below one pixel footprint at the surface
    gx, gy = np.meshgrid(np.arange(-3.0, 3.0, 0.0125), np.arange(-2.0, 2.0, 0.0125))
    plane = np.stack((gx, gy, (R.PLANE_C - R.PLANE_N[0] * gx - R.PLANE_N[1] * gy) / R.PLANE_N[2]), axis=-1).reshape(-1, 3)
    k = np.arange(20000) + 0.5
    phi, theta = np.arccos(1 - 2 * k / 20000), math.pi * (1 + 5 ** 0.5) * k
    sphere = R.SPHERE_O + R.SPHERE_R * np.stack((np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)), axis=1)
    gt = torch.from_numpy(np.concatenate((plane, sphere)).astype(np.float32)).to(dev)
    footprint = float(ranges.min()) / 152.0            # the nearest point under the longest focal length
    result = evaluate_points(xyz, gt)
    print(f"[mvs] fused cloud against {gt.shape[0]} sampled surface points: accuracy {result['accuracy']:.4f}, "
          f"pixel footprint {footprint:.4f}")
    assert result["accuracy"] < footprint


def test_bad_arguments_through_the_raw_abi_leave_the_outputs_untouched(gpu_device):
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    dev = gpu_device
    _, depth, _, _, rows, (fx, fy) = _scene()
    d = torch.from_numpy(depth).to(dev)
    table, keep = _table(rows, dev)
    count = torch.full((37, 70), 7, dtype=torch.uint8, device=dev)
    fused = torch.full((37, 70), -1.0, device=dev)
    xyz = torch.full((37 * 70, 3), -1.0, device=dev)
    c2w = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1))
    good = dict(depth=d.data_ptr(), H=37, W=70, fx=float(fx), fy=float(fy), sources=table.data_ptr(), S=4, pix=1.0, dep=0.01,
                mv=2, count=count.data_ptr(), fused=fused.data_ptr())
    inf, nan = math.inf, math.nan
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        call = lambda **kw: lib.gsr_mvs_consistency(*{**good, **kw}.values(), stream)      # noqa: E731
        for kw in ({"depth": None}, {"count": None}, {"fused": None}, {"H": 0}, {"W": -1}, {"S": -1}, {"S": 65},
                   {"sources": None}, {"fx": 0.0}, {"fy": inf}, {"pix": nan}, {"pix": 0.0}, {"dep": -1.0}, {"dep": inf},
                   {"mv": -1}):
            assert call(**kw) == -1, kw
        for kw in ({"depth": good["depth"] + 2}, {"fused": good["fused"] + 2}, {"sources": good["sources"] + 4}):
            assert call(**kw) == -3, kw
        back = lambda **kw: lib.gsr_depth_backproject(*{**dict(depth=d.data_ptr(), H=37, W=70, fx=float(fx), fy=float(fy),     # noqa: E731
                                                               m=C.addressof(c2w), xyz=xyz.data_ptr()), **kw}.values(), stream)
        for kw in ({"depth": None}, {"xyz": None}, {"m": None}, {"H": -1}, {"fx": nan}, {"fy": 0.0}):
            assert back(**kw) == -1, kw
        assert back(xyz=xyz.data_ptr() + 2) == -3 and back(H=0) == 0
        torch.cuda.synchronize()
        assert bool((count == 7).all()) and bool((fused == -1).all()) and bool((xyz == -1).all())
        # and the same arguments, well-formed, do the work
        assert call() == 0 and back() == 0
        torch.cuda.synchronize()
    assert int(count.max()) == 3 and bool((fused >= 0).all()) and bool((xyz[:, 2] >= 0).all())
    del keep
