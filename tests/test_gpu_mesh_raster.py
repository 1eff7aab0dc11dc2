"""The mesh rasterizer on the device (csrc/mesh_raster.hip; ``mesh.rasterize_mesh``, ``mesh.face_view_counts``,
``mesh.cull_invisible_faces``, ``mesh.face_normal_map``) against the numpy restatement
(tests/mesh_raster_restate.py): depth bits and face ids equal on every pixel of the inputs that are exact in float32, on
every pixel that is not fragile of the general one; the queue and its drain; independence of the order of the faces;
visibility counts and the culling on top; and a fused sphere end to end."""
import numpy as np
import pytest
import torch

import mesh_raster_restate as R

pytestmark = pytest.mark.gpu

_wants = {}


def want(name, make, cull=False):
    """A scene of the restatement and its result, computed once."""
    if (name, cull) not in _wants:
        s = make()
        _wants[(name, cull)] = (s, R.rasterize(s.vertices, s.faces, s.cam, s.near, cull))
    return _wants[(name, cull)]


def on_device(s, dev):
    return torch.from_numpy(s.vertices).to(dev), torch.from_numpy(s.faces).to(dev)


def bits(t):
    return t.cpu().numpy().view(np.int32)


def assert_equal(got, r, where=None, what=""):
    depth, face_id = got[0], got[1]
    assert depth.dtype == torch.float32 and face_id.dtype == torch.int32 and depth.shape == face_id.shape == r.depth.shape
    where = np.ones(r.depth.shape, dtype=bool) if where is None else where
    d_off = (bits(depth) != r.depth.view(np.int32)) & where
    i_off = (face_id.cpu().numpy() != r.face_id) & where
    print(f"[mesh_raster] {what}: depth bits off on {int(d_off.sum())}, ids off on {int(i_off.sum())} of {int(where.sum())} pixels")
    assert not d_off.any() and not i_off.any(), what


def test_one_triangle_on_an_8_by_8_image(gpu_device):
    from mvs_gaussian_splatting_amd import rasterize_mesh
    cam, _ = R.dyadic_camera(8, 8, 16.0)
    tri = np.array((((-3.0) / 16, (-2.5) / 16, 1.0), (5.25 / 8, (-1.0) / 8, 2.0), ((-1.0) / 4, 3.5 / 4, 4.0)))
    vertices, faces = R.soup_mesh(tri[None])
    s = R.types.SimpleNamespace(vertices=vertices, faces=faces, cam=cam, near=R.NEAR)
    r = R.rasterize(vertices, faces, cam, R.NEAR)
    assert 8 <= (r.face_id == 0).sum() < 64 and len(np.unique(r.depth)) > 6
    got = rasterize_mesh(*on_device(s, gpu_device), cam, near=R.NEAR)
    assert_equal(got, r, what="one triangle")
    assert_equal(rasterize_mesh(*on_device(s, gpu_device), cam, near=R.NEAR, cull_backfaces=True),
                 R.rasterize(vertices, faces, cam, R.NEAR, True), what="one triangle, back faces culled")


@pytest.mark.parametrize("name,make", [("dyadic", R.dyadic_soup), ("dyadic_permuted", lambda: R.dyadic_soup(permute=True, seed=4))])
@pytest.mark.parametrize("cull", [False, True])
def test_dyadic_soup_is_the_restatements_everywhere(gpu_device, name, make, cull):
    """2000 triangles on 97 x 61 (the width no multiple of 64): behind the camera, crossing near with one and with two
    corners inside, without area, a NaN corner, coincident duplicates.  The inputs are exact, so every pixel counts."""
    from mvs_gaussian_splatting_amd import rasterize_mesh
    s, r = want(name, make, cull)
    depth, face_id, stats = rasterize_mesh(*on_device(s, gpu_device), s.cam, near=s.near, cull_backfaces=cull, stats=True)
    assert_equal((depth, face_id), r, what=f"{name}, cull_backfaces={cull}")
    assert stats == {"dropped": r.dropped, "bad_faces": 0} and r.dropped == 2


def test_general_soup_is_the_restatements_off_the_fragile_pixels(gpu_device):
    from mvs_gaussian_splatting_amd import rasterize_mesh
    s, r = want("general", R.general_soup)
    fragile = R.fragile_pixels(s.vertices, s.faces, s.cam, s.near)
    covered = r.layers > 0
    share = fragile.sum() / covered.sum()
    print(f"[mesh_raster] general soup: {int(fragile.sum())} fragile of {int(covered.sum())} covered pixels ({100 * share:.3f} %)")
    assert share < 0.01
    got = rasterize_mesh(*on_device(s, gpu_device), s.cam, near=s.near)
    everywhere = (bits(got[0]) != r.depth.view(np.int32)) | (got[1].cpu().numpy() != r.face_id)
    print(f"[mesh_raster] general soup: {int(everywhere.sum())} pixels differ anywhere, fragile ones included")
    assert_equal(got, r, ~fragile, "general soup, pixels that are not fragile")


def test_large_pieces_go_through_the_queue(gpu_device):
    """One triangle over a whole 70 x 50 image behind 400 small ones; and 300 triangles with 24 x 24-pixel boxes on 64 x 48:
    more queued pieces than the GSR_RASTER_DRAIN_WAVES = 256 that one pass of the drain grid takes (64 workgroups of four
    waves, one piece per wave), so every wave strides."""
    from mvs_gaussian_splatting_amd import _lib, rasterize_mesh
    assert (_lib.RASTER_LANE_PIXELS, _lib.RASTER_DRAIN_WAVES) == (R.LANE_PIXELS, R.DRAIN_WAVES) == (16, 256)
    s, r = want("big", R.big_triangle_scene)
    assert r.queued >= 1 and (r.face_id == s.big).sum() > 1000
    assert_equal(rasterize_mesh(*on_device(s, gpu_device), s.cam, near=s.near), r, what="one triangle over the whole image")
    s, r = want("queued", R.queued_scene)
    assert r.queued > R.DRAIN_WAVES
    for cull in (False, True):
        _, rc = want("queued", R.queued_scene, cull)
        assert_equal(rasterize_mesh(*on_device(s, gpu_device), s.cam, near=s.near, cull_backfaces=cull), rc,
                     what=f"{r.queued} queued pieces, cull_backfaces={cull}")


def test_the_result_does_not_depend_on_the_order_of_the_faces(gpu_device):
    from mvs_gaussian_splatting_amd import _lib, rasterize_mesh
    dev = gpu_device
    s, r = want("dyadic", R.dyadic_soup)
    vertices, faces = on_device(s, dev)
    first = rasterize_mesh(vertices, faces, s.cam, near=s.near)
    again = rasterize_mesh(vertices, faces, s.cam, near=s.near)
    assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(first[1], again[1])
    perm = np.random.default_rng(1).permutation(len(s.faces))          # new face k is old face perm[k]
    shuffled = rasterize_mesh(vertices, torch.from_numpy(s.faces[perm]).to(dev), s.cam, near=s.near)
    assert torch.equal(shuffled[0].view(torch.int32), first[0].view(torch.int32)), "depth is the same bits"
    # ids map through the permutation wherever no two faces tie for the pixel's depth
    tie = np.zeros(r.depth.shape, dtype=bool)
    for f, mine in enumerate(R.pieces_of(s.vertices, s.faces, s.cam, s.near)):
        for piece in mine:
            if piece is not None:
                iy, ix, z = R.cover(piece, *r.depth.shape[::-1])
                tie[iy, ix] |= (z.view(np.int32) == r.depth.view(np.int32)[iy, ix]) & (r.face_id[iy, ix] != f)
    ids = shuffled[1].cpu().numpy()
    mapped = np.where(ids >= 0, perm[np.maximum(ids, 0)], -1)
    assert tie.sum() > 10 and (~tie).sum() > 1000
    assert np.array_equal(mapped[~tie], r.face_id[~tie])
    assert np.array_equal(ids >= 0, r.face_id >= 0)
    # through the entry points, into arrays full of garbage: every pixel of both outputs is written
    lib = _lib.load()
    H, W = r.depth.shape
    row = _lib.GsrCullView()
    row.width, row.height, row.fx, row.fy = W, H, *(float(v) for v in R.focal(s.cam)[2:])
    row.world_to_view[:] = s.cam.world_view_transform.reshape(-1).tolist()
    keys = torch.full((H * W,), 0x0123456789ABCDEF, dtype=torch.int64, device=dev)
    qbytes = lib.gsr_raster_queue_bytes(len(s.faces))
    queue = torch.full((qbytes,), 0xA5, dtype=torch.uint8, device=dev)
    depth = torch.full((H, W), float("nan"), device=dev)
    face_id = torch.full((H, W), -77, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    import ctypes as C
    _lib.check(lib.gsr_raster_view(vertices.data_ptr(), len(s.vertices), faces.data_ptr(), len(s.faces), C.byref(row), s.near,
                                   _lib.RASTER_CLEAR, keys.data_ptr(), queue.data_ptr(), qbytes, None, stream), "view")
    _lib.check(lib.gsr_raster_resolve(keys.data_ptr(), H, W, depth.data_ptr(), face_id.data_ptr(), stream), "resolve")
    assert torch.equal(depth.view(torch.int32), first[0].view(torch.int32)) and torch.equal(face_id, first[1])
    assert np.array_equal(keys.cpu().numpy().view(np.uint64).reshape(H, W), r.keys)
    # the same keys without the load in front of the atomic, and with the corners taken to view space first
    for flags, scratch in ((_lib.RASTER_CLEAR | _lib.RASTER_NO_LOAD_SKIP, None),
                           (_lib.RASTER_CLEAR, torch.empty((len(s.vertices), 3), device=dev))):
        other = torch.empty_like(keys)
        _lib.check(lib.gsr_raster_view(vertices.data_ptr(), len(s.vertices), faces.data_ptr(), len(s.faces), C.byref(row),
                                       s.near, flags, other.data_ptr(), queue.data_ptr(), qbytes,
                                       None if scratch is None else scratch.data_ptr(), stream), "view")
        assert torch.equal(other, keys)


def _quads():
    """Three parallel quads at z = -1, 0, 1 (each two faces), the outer ones facing the cameras on either side."""
    sq = lambda z: R.quad(((-1.0, -1.0, z), (1.0, -1.0, z), (1.0, 1.0, z), (-1.0, 1.0, z)))           # noqa: E731
    vertices, faces = R.soup_mesh(np.concatenate((sq(-1.0), sq(0.0), sq(1.0))))
    front = R.camera(R.look_at((0.0, 0.0, -4.0), (0.0, 0.0, 0.0)), 40, 30, 32.0, 32.0)
    back = R.camera(R.look_at((0.0, 0.0, 4.0), (0.0, 0.0, 0.0)), 36, 36, 32.0, 32.0)
    return vertices, faces, [front, back]


def test_visibility_counts_and_the_cull_on_two_quads_and_one_between(gpu_device):
    from mvs_gaussian_splatting_amd import cull_invisible_faces, face_view_counts
    dev = gpu_device
    vertices, faces, cams = _quads()
    want_counts = R.face_counts(vertices, faces, cams, R.NEAR)
    assert want_counts.tolist() == [1, 1, 0, 0, 1, 1]
    v, f = torch.from_numpy(vertices).to(dev), torch.from_numpy(faces).to(dev)
    colors = torch.rand(len(vertices), 3, device=dev)
    counts = face_view_counts(v, f, cams, near=R.NEAR)
    assert counts.dtype == torch.int32 and counts.tolist() == [1, 1, 0, 0, 1, 1]
    assert torch.equal(face_view_counts(v, f, cams, near=R.NEAR), counts)
    chunked = face_view_counts(v, f, cams[:1], near=R.NEAR)
    assert chunked.tolist() == [1, 1, 0, 0, 0, 0]
    both = face_view_counts(v, f, cams[1:], near=R.NEAR, counts=chunked)
    assert both is chunked and torch.equal(both, counts)
    assert face_view_counts(v, f, cams + cams, near=R.NEAR).tolist() == [2, 2, 0, 0, 2, 2], "once per view, however many pixels"
    out_v, out_f, out_c, n = cull_invisible_faces(v, f, colors, cameras=cams, near=R.NEAR, return_counts=True)
    keep = np.array([0, 1, 2, 3, 4, 5, 12, 13, 14, 15, 16, 17])
    assert torch.equal(n, counts)
    assert np.array_equal(bits(out_v), vertices[keep].view(np.int32)) and torch.equal(out_c, colors[torch.from_numpy(keep).to(dev)])
    assert out_f.tolist() == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]]
    plain = cull_invisible_faces(v, f, cameras=[], counts=counts.clone(), near=R.NEAR)
    assert len(plain) == 3 and plain[2] is None and torch.equal(plain[0], out_v) and torch.equal(plain[1], out_f)
    assert cull_invisible_faces(v, f, cameras=cams, near=R.NEAR, min_views=2)[1].shape == (0, 3)
    assert cull_invisible_faces(v, f, cameras=cams, near=R.NEAR, min_views=0)[1].shape == (6, 3)


def test_edges_no_faces_no_cameras_and_a_camera_that_sees_nothing(gpu_device):
    from mvs_gaussian_splatting_amd import cull_invisible_faces, face_normal_map, face_view_counts, rasterize_mesh
    dev = gpu_device
    vertices, faces, cams = _quads()
    v, f = torch.from_numpy(vertices).to(dev), torch.from_numpy(faces).to(dev)
    for vv, ff in ((v, f[:0]), (v[:0], f[:0])):
        depth, face_id, stats = rasterize_mesh(vv, ff, cams[0], stats=True)
        assert tuple(depth.shape) == (30, 40) and not depth.any() and (face_id == -1).all() and stats == {"dropped": 0, "bad_faces": 0}
        assert tuple(face_view_counts(vv, ff, cams).shape) == (0,)
        out = cull_invisible_faces(vv, ff, cameras=cams, return_counts=True)
        assert tuple(out[0].shape) == tuple(out[1].shape) == (0, 3) and out[2] is None and tuple(out[3].shape) == (0,)
    assert face_view_counts(v, f, []).tolist() == [0] * 6
    away = R.camera(R.look_at((0.0, 0.0, -4.0), (0.0, 0.0, -8.0)), 33, 17, 20.0, 20.0)
    depth, face_id = rasterize_mesh(v, f, away)
    assert not depth.any() and (face_id == -1).all() and face_view_counts(v, f, [away]).tolist() == [0] * 6
    assert not face_normal_map(v, f, face_id, away).any()
    # a face index out of range is skipped and counted, never used
    broken = f.clone()
    broken[1, 2] = len(vertices)
    broken[4, 0] = -1
    depth, face_id, stats = rasterize_mesh(v, broken, cams[0], near=R.NEAR, stats=True)
    owners = set(face_id.unique().tolist())
    assert stats == {"dropped": 0, "bad_faces": 2} and {-1, 0, 3} <= owners and not owners & {1, 4}, "face 3 shows through"
    # normals of the front quad: (0, 0, -1) in view space wherever it owns the pixel
    depth, face_id = rasterize_mesh(v, f, cams[0], near=R.NEAR)
    n = face_normal_map(v, f, face_id, cams[0])
    hit = face_id >= 0
    assert hit.sum() > 200 and torch.allclose(n[:, hit], torch.tensor([0.0, 0.0, -1.0], device=dev)[:, None].expand(3, int(hit.sum())))
    assert not n[:, ~hit].any()


def test_a_fused_sphere_end_to_end(gpu_device):
    """The analytic depth of the unit sphere from six views into a 32^3 volume, extracted, and rasterized from the views:
    a face on every pixel of the silhouette eroded by one pixel, the depth within sqrt(3) voxels of the analytic one (the
    bound on a TSDF vertex's distance from the surface), and the faces no view sees -- the back of the truncation band --
    removed without changing a bit of any view's depth map."""
    from mvs_gaussian_splatting_amd import TSDFVolume, cull_invisible_faces, face_view_counts, rasterize_mesh
    dev = gpu_device
    c = R.sphere_case()
    volume = TSDFVolume(c.origin, c.voxel_size, c.dims, c.sdf_trunc, with_color=False, device=dev)
    for cam, depth in zip(c.cameras, c.depths):
        volume.integrate(torch.from_numpy(depth).to(dev), cam)
    vertices, faces, _ = volume.extract_mesh()
    assert len(faces) > 5000
    before = [rasterize_mesh(vertices, faces, cam) for cam in c.cameras]
    depth, face_id = (t.cpu().numpy() for t in before[0])
    inside = R.erode(c.masks[0])
    err = np.abs(depth - c.depths[0])[inside]
    print(f"[mesh_raster] sphere: {len(faces)} faces; {int(inside.sum())} pixels in the eroded silhouette, "
          f"{int((face_id[inside] < 0).sum())} without a face; depth off by at most {err.max():.4f} (bound {np.sqrt(3) * c.voxel_size:.4f})")
    assert inside.sum() > 300 and (face_id[inside] >= 0).all()
    assert err.max() <= np.sqrt(3) * c.voxel_size
    counts = face_view_counts(vertices, faces, c.cameras)
    v2, f2, _ = cull_invisible_faces(vertices, faces, cameras=c.cameras, min_views=1)
    assert 0 < len(f2) < len(faces) and len(f2) == int((counts > 0).sum())
    print(f"[mesh_raster] sphere: {len(f2)} of {len(faces)} faces seen by some view")
    for cam, (d0, _) in zip(c.cameras, before):
        d1, _ = rasterize_mesh(v2, f2, cam)
        assert torch.equal(d1.view(torch.int32), d0.view(torch.int32))
