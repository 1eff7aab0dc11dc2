"""TSDF fusion in contracted space on the HIP path (csrc/tsdf.hip, ABI v33; ``tsdf.ContractedTSDFVolume``)
against the float64 restatement of tests/tsdf_contracted_restate.py.

Shapes: a 70 x 9 x 6 volume (past one 64-wide x-chunk, ragged tail) on a dyadic grid that holds q = 0, |q| = 1, |q| = q_max
and |q| = 2 exactly and corners beyond 2, under two 48 x 40 views; the 33^3 sphere beyond the unit ball of the host test.
Bars as tests/test_gpu_tsdf.py: integration on the points none of whose float64 comparisons is within
tsdf_restate.MARGIN of flipping (tests/test_tsdf_contracted_host.py caps their share), ``weight`` exactly, ``tsdf`` and
``color`` max-norm within max(1e-5, 2 x the float32 restatement's own error against float64); mesh faces integer for
integer; world-space vertices within the same bar relative to the mesh's extent.  The observed figures are printed (-s).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import small_scene
import tsdf_restate as R
import tsdf_contracted_restate as CR

pytestmark = pytest.mark.gpu


def _bar(ref32, ref64, scale=1.0):
    return max(1e-5, 2.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()) / scale)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _case():
    return CR.integration_case()


@functools.lru_cache(maxsize=None)
def _reference(with_color, max_weight):
    """float64 and float32 restatement of the two views; computed once, never modified."""
    _, views = _case()
    return CR.run_case(views, with_color, max_weight), CR.run_case(views, with_color, max_weight, np.float32)


def _volume(dev, with_color):
    from mvs_gaussian_splatting_amd import ContractedTSDFVolume
    return ContractedTSDFVolume(CR.CASE_ORIGIN, CR.CASE_VOXEL, CR.CASE_DIMS, CR.CASE_TRUNC, CR.CASE_CENTER, CR.CASE_RADIUS,
                                q_max=CR.CASE_Q_MAX, with_color=with_color, device=dev)


def _integrate(vol, cameras, views, max_weight):
    dev = vol.tsdf.device
    for cam, view in zip(cameras, views):
        vol.integrate(torch.from_numpy(view["depth"]).to(dev), cam,
                      color=torch.from_numpy(view["color"]).to(dev) if vol.with_color else None, weight=view["weight"],
                      max_depth=view["max_depth"], max_weight=max_weight)
    return vol


@pytest.mark.parametrize("with_color,max_weight", [(True, None), (False, None), (True, CR.CASE_MAX_WEIGHT)])
def test_contracted_integration_matches_the_float64_restatement(gpu_device, with_color, max_weight):
    (ref, touched, fragile), (ref32, _, _) = _reference(with_color, max_weight)
    cameras, views = _case()
    vol = _integrate(_volume(gpu_device, with_color), cameras, views, max_weight)
    again = _integrate(_volume(gpu_device, with_color), cameras, views, max_weight)
    start = _volume(gpu_device, with_color)
    ok = ~fragile
    got_w = vol.weight.cpu().numpy()
    assert np.array_equal(got_w[ok], ref["weight"][ok].astype(np.float32)), "weights differ on robust points"
    if max_weight is not None:
        assert got_w.max() == max_weight and int((got_w == max_weight).sum()) > 50
    for name in ("tsdf", "color") if with_color else ("tsdf",):
        got = getattr(vol, name).cpu().numpy().astype(np.float64)
        err = float(np.abs(got - ref[name])[ok].max())
        bar = _bar(ref32[name][ok], ref[name][ok])
        print(f"[tsdf contracted] color={with_color} max_weight={max_weight} {name}: max error {err:.2e}, bar {bar:.2e}, "
              f"{int(touched.sum())} updated points, {int(fragile.sum())} left out")
        assert err <= bar, f"{name}: {err:.3e} > {bar:.3e}"
    m = np.sqrt(CR.squared_norm(CR.grid_points(CR.CASE_DIMS, CR.CASE_ORIGIN, CR.CASE_VOXEL)))
    outside = torch.from_numpy(m >= CR.CASE_Q_MAX).to(gpu_device)            # exact on the dyadic grid, |q| = q_max included
    idle = torch.from_numpy(~touched & ok).to(gpu_device)
    assert int(outside.sum()) > 200 and int((idle & ~outside).sum()) > 100
    for name in ("tsdf", "weight") + (("color",) if with_color else ()):
        got, first = getattr(vol, name), getattr(start, name)
        assert _same_bits(got[outside], first[outside]), f"{name} of a point with |q| >= q_max was written"
        assert _same_bits(got[idle], first[idle]), f"{name} of a skipped point was written"
        assert _same_bits(got, getattr(again, name)), f"{name} differs from run to run"


def test_the_unit_ball_is_the_identity(gpu_device):
    """Every |q| <= 1, center 0, radius 1: the contracted kernel is the plain one bit for bit -- one body."""
    from mvs_gaussian_splatting_amd import ContractedTSDFVolume, TSDFVolume
    cameras, views = CR.ball_case()
    for with_color in (True, False):
        plain = TSDFVolume(CR.BALL_ORIGIN, CR.BALL_VOXEL, CR.BALL_DIMS, CR.BALL_TRUNC, with_color=with_color, device=gpu_device)
        ball = ContractedTSDFVolume(CR.BALL_ORIGIN, CR.BALL_VOXEL, CR.BALL_DIMS, CR.BALL_TRUNC, (0.0, 0.0, 0.0), 1.0,
                                    with_color=with_color, device=gpu_device)
        for vol in (plain, ball):
            _integrate(vol, cameras, views, CR.CASE_MAX_WEIGHT)
        updated = int((plain.weight > 0).sum())
        print(f"[tsdf contracted] unit ball color={with_color}: {updated} of {plain.weight.numel()} points updated, "
              f"{int((plain.tsdf < 0).sum())} inside, largest weight {float(plain.weight.max())}")
        assert updated > 1000 and int((plain.weight == 0).sum()) > 100 and int((plain.tsdf < 0).sum()) > 100
        for name in ("tsdf", "weight") + (("color",) if with_color else ()):
            assert _same_bits(getattr(ball, name), getattr(plain, name)), name


def _load(field, dev, contracted=True):
    from mvs_gaussian_splatting_amd import ContractedTSDFVolume, TSDFVolume
    nz, ny, nx = field["tsdf"].shape
    with_color = field["color"] is not None
    if contracted:
        vol = ContractedTSDFVolume(field["origin"], field["voxel_size"], (nx, ny, nz), field["sdf_trunc"], field["center"],
                                   field["radius"], q_max=field["q_max"], with_color=with_color, device=dev)
    else:
        vol = TSDFVolume(field["origin"], field["voxel_size"], (nx, ny, nz), field["sdf_trunc"], with_color=with_color,
                         device=dev)
    vol.tsdf = torch.from_numpy(field["tsdf"]).to(dev)
    vol.weight = torch.from_numpy(field["weight"]).to(dev)
    if with_color:
        vol.color = torch.from_numpy(field["color"]).to(dev)
    return vol


@functools.lru_cache(maxsize=None)
def _shell_reference():
    field = CR.shell_sphere_field(with_color=True)
    return field, CR.extract(field), CR.extract(field, dtype=np.float32)


def test_extraction_is_the_base_mesh_with_uncontracted_vertices(gpu_device):
    field, (rv, rf, rc), (rv32, _, _) = _shell_reference()
    vol, base = _load(field, gpu_device), _load(field, gpu_device, contracted=False)
    bv, bf, bc = base.extract_mesh()
    gv, gf, gc = vol.extract_mesh(contracted=True)
    vertices, faces, colors = vol.extract_mesh()
    assert vertices.dtype == torch.float32 and faces.dtype == torch.int32 and colors.dtype == torch.float32
    assert torch.equal(faces, bf) and torch.equal(gf, bf), "faces differ from the base extraction"
    assert np.array_equal(faces.cpu().numpy(), rf), "faces differ from the restatement"
    assert _same_bits(gv, bv) and _same_bits(gc, bc) and _same_bits(colors, bc)
    assert not torch.equal(vertices, bv), "the vertices were not uncontracted"
    v = vertices.cpu().numpy().astype(np.float64)
    ext = float(np.abs(rv - np.array(CR.SHELL_CENTER)).max())
    err, bar = float(np.abs(v - rv).max()) / ext, _bar(rv32, rv, ext)
    print(f"[tsdf contracted] shell sphere: V {len(v)} F {len(rf)}, world vertex error {err:.2e} of the extent {ext:.2f} "
          f"(bar {bar:.2e})")
    assert err <= bar
    R.assert_closed_oriented_sphere(v, faces.cpu().numpy())
    off = np.abs(np.linalg.norm(v - np.array(CR.SHELL_CENTER), axis=1) - CR.SHELL_SPHERE)
    assert off.max() < 0.1
    v2, f2, c2 = vol.extract_mesh()
    assert _same_bits(v2, vertices) and torch.equal(f2, faces) and _same_bits(c2, colors)


def test_contracted_volume_without_a_crossing_gives_empty_tensors(gpu_device):
    from mvs_gaussian_splatting_amd import ContractedTSDFVolume
    for with_color in (True, False):
        vol = ContractedTSDFVolume((-1.5, -1.5, -1.5), 0.5, (7, 7, 7), 1.0, (0.0, 0.0, 0.0), 2.0, with_color=with_color,
                                   device=gpu_device)
        vol.weight.fill_(1.0)
        for contracted in (False, True):
            vertices, faces, colors = vol.extract_mesh(contracted=contracted)
            assert tuple(vertices.shape) == (0, 3) and tuple(faces.shape) == (0, 3) and faces.dtype == torch.int32
            assert (colors is None) != with_color and (colors is None or tuple(colors.shape) == (0, 3))
    torch.cuda.synchronize()


def test_uncontract_points_through_the_raw_abi(gpu_device):
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    con = _lib.GsrTsdfContraction()
    con.center[0], con.center[1], con.center[2] = CR.CASE_CENTER
    con.radius, con.q_max = CR.CASE_RADIUS, 1.9
    rng = np.random.default_rng(9)
    d = rng.normal(size=(66, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rows = (d * rng.uniform(0.0, 1.9, 66)[:, None]).astype(np.float32)
    rows[0], rows[1], rows[2], rows[3] = (0, 0, 0), (0, -1, 0), (np.float32(1.9), 0, 0), (0.6, 0, -0.8)
    assert lib.gsr_tsdf_uncontract_points(None, 0, C.byref(con), None) == 0
    with torch.cuda.device(gpu_device):
        stream = torch.cuda.current_stream(gpu_device).cuda_stream
        for n in (0, 1, 65):
            start = 0 if n != 1 else 2                                     # n = 1: the row at |q| = 1.9
            xyz = torch.from_numpy(rows[start:]).to(gpu_device).contiguous()
            assert lib.gsr_tsdf_uncontract_points(xyz.data_ptr(), n, C.byref(con), stream) == 0
            got = xyz.cpu().numpy()
            assert np.array_equal(got[n:], rows[start + n:]), "a row at or beyond n was written"
            if n == 0:
                continue
            ref = CR.uncontract(rows[start:start + n], CR.CASE_CENTER, CR.CASE_RADIUS)
            ref32 = CR.uncontract(rows[start:start + n], CR.CASE_CENTER, CR.CASE_RADIUS, np.float32)
            scale = float(np.abs(ref - np.array(CR.CASE_CENTER)).max())
            err, bar = float(np.abs(got[:n] - ref).max()) / scale, _bar(ref32, ref, scale)
            print(f"[tsdf contracted] uncontract n={n}: error {err:.2e} of {scale:.2f} (bar {bar:.2e})")
            assert err <= bar
            if n == 65:                                                   # inside the unit ball: center + radius * q exactly
                inner = CR.uncontract(rows[[0, 1, 3]], CR.CASE_CENTER, CR.CASE_RADIUS, np.float32)
                assert np.array_equal(got[[0, 1, 3]], inner) and np.array_equal(got[0], np.float32(CR.CASE_CENTER))


def test_bad_arguments_through_the_raw_abi_leave_the_fields_untouched(gpu_device):
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    cameras, views = _case()
    vol = _integrate(_volume(gpu_device, True), cameras, views[:1], None)
    keep = {n: getattr(vol, n).clone() for n in ("tsdf", "weight", "color")}
    native, con, view = vol._native(), vol._native_contraction(), _lib.GsrTsdfView()
    depth = torch.from_numpy(views[1]["depth"]).to(gpu_device)
    color = torch.from_numpy(views[1]["color"]).to(gpu_device)
    M = cameras[1].world_view_transform.to(gpu_device).float().contiguous()
    view.width, view.height, view.fx, view.fy = CR.CASE_W, CR.CASE_H, views[1]["fx"], views[1]["fy"]
    view.weight, view.max_depth, view.max_weight = 1.0, float("inf"), float("inf")
    view.viewmatrix, view.depth, view.color = M.data_ptr(), depth.data_ptr(), color.data_ptr()
    verts = torch.rand(8, 3, device=gpu_device)
    verts_keep = verts.clone()
    with torch.cuda.device(gpu_device):
        stream = torch.cuda.current_stream(gpu_device).cuda_stream
        for field, bad in (("radius", 0.0), ("radius", float("nan")), ("radius", float("inf")), ("q_max", 1.0),
                           ("q_max", 2.0), ("q_max", float("nan"))):
            good = getattr(con, field)
            setattr(con, field, bad)
            assert lib.gsr_tsdf_integrate_contracted(C.byref(native), C.byref(con), C.byref(view), stream) == -1, (field, bad)
            assert lib.gsr_tsdf_uncontract_points(verts.data_ptr(), 8, C.byref(con), stream) == -1, (field, bad)
            setattr(con, field, good)
        assert lib.gsr_tsdf_integrate_contracted(C.byref(native), None, C.byref(view), stream) == -1
        assert lib.gsr_tsdf_integrate_contracted(None, C.byref(con), C.byref(view), stream) == -1
        assert lib.gsr_tsdf_integrate_contracted(C.byref(native), C.byref(con), None, stream) == -1
        assert lib.gsr_tsdf_uncontract_points(verts.data_ptr(), 8, None, stream) == -1
        assert lib.gsr_tsdf_uncontract_points(None, 8, C.byref(con), stream) == -1
        assert lib.gsr_tsdf_uncontract_points(verts.data_ptr(), -1, C.byref(con), stream) == -1
        torch.cuda.synchronize()
        assert all(_same_bits(getattr(vol, n), keep[n]) for n in keep) and _same_bits(verts, verts_keep)
        # and the same structs, well-formed, do the work
        assert lib.gsr_tsdf_integrate_contracted(C.byref(native), C.byref(con), C.byref(view), stream) == 0
        torch.cuda.synchronize()
    assert not torch.equal(vol.weight, keep["weight"])


def test_fuse_views_into_a_contracted_volume_equals_the_hand_filled_one_and_leaves_the_frame_path_alone(gpu_device):
    from mvs_gaussian_splatting_amd import ContractedTSDFVolume, fuse_views, render, surface_depth
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    dev = gpu_device
    model, cam0, bg, _ = small_scene(scale=0.08)
    cameras = [cam0.to(dev)] + [small_scene(P=1, view=v)[1].to(dev) for v in (1, 3)]
    model.to(dev)
    bg, pipe = bg.to(dev), PipelineParams()
    make = lambda: ContractedTSDFVolume((-1.9,) * 3, 3.8 / 32, (33, 33, 33), 5 * 1.25 * 3.8 / 32, (0.0, 0.0, 5.5), 1.25,  # noqa: E731
                                        device=dev)
    with torch.no_grad():
        before = render(cameras[1], model, pipe, bg, return_depth=True)
    fused = fuse_views(cameras, model, pipe, bg, make(), alpha_min=0.5, max_depth=7.5)
    blended = fuse_views(cameras, model, pipe, bg, make(), alpha_min=0.5, depth_ratio=0.5)
    by_hand, by_hand_blended = make(), make()
    with torch.no_grad():
        for cam in cameras:
            pkg = render(cam, model, pipe, bg, return_depth=True)
            expected = torch.where(pkg["alpha"] >= 0.5, pkg["depth"] / pkg["alpha"], torch.zeros_like(pkg["depth"]))
            by_hand.integrate(expected, cam, color=pkg["render"], max_depth=7.5)
            pkg = render(cam, model, pipe, bg, return_depth=True, return_median_depth=True)
            by_hand_blended.integrate(surface_depth(pkg["depth"], pkg["alpha"], pkg["median_depth"], 0.5, 0.5), cam,
                                      color=pkg["render"])
        after = render(cameras[1], model, pipe, bg, return_depth=True)
    updated = int((fused.weight > 0).sum())
    far = int((fused.weight.cpu().numpy() > 0)[np.sqrt(CR.squared_norm(CR.grid_points((33,) * 3, (-1.9,) * 3, 3.8 / 32))) > 1].sum())
    print(f"[tsdf contracted] fuse_views: {updated} of {fused.weight.numel()} points updated, {far} of them beyond the unit "
          f"ball, largest weight {float(fused.weight.max())}")
    assert updated > 1000 and far > 100
    for name in ("tsdf", "weight", "color"):
        assert torch.equal(getattr(fused, name), getattr(by_hand, name)), name
        assert torch.equal(getattr(blended, name), getattr(by_hand_blended, name)), f"{name} with depth_ratio"
    for name in ("render", "depth", "invdepth", "alpha", "radii"):
        assert torch.equal(before[name], after[name]), f"{name} of the same frame changed across the fusion"
