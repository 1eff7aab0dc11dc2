"""The view culling on the device (csrc/mesh_cull.hip; ``mesh.vertex_view_counts``, ``mesh.cull_mesh_by_views``,
``mesh.dilate_mask``, ``tsdf.view_counts_for_views``) against the numpy restatement
(tests/mesh_cull_restate.py): the counts exact on every pair that float32 decides (and within the number of fragile views
of the vertex elsewhere), exact everywhere on the dyadic case, the same bits in chunks and on a second run; the dilation
exact; the culling end to end; and the rendering glue on a small scene."""
import numpy as np
import pytest
import torch

from conftest import small_scene
import mesh_cull_restate as R

pytestmark = pytest.mark.gpu

_scenes = {}


def scene(S):
    """The restatement's scene with S views and its float64 counts, computed once."""
    if S not in _scenes:
        s = R.scene(S)
        s.want = R.counts(s.vertices, s.cameras, s.masks, s.depths, s.near, s.depth_tol, dtype=np.float64)
        _scenes[S] = s
    return _scenes[S]


def on_device(s, dev):
    maps = lambda group: [None if m is None else torch.from_numpy(np.ascontiguousarray(m)).to(dev) for m in group]   # noqa: E731
    return torch.from_numpy(s.vertices).to(dev), maps(s.masks), maps(s.depths)


def garbage(V, dev):
    return (torch.full((V,), -77, dtype=torch.int32, device=dev), torch.full((V,), 1 << 20, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("S", [0, 1, 5, 70])
def test_counts_are_the_restatements(gpu_device, S):
    from mvs_gaussian_splatting_amd import _lib, vertex_view_counts
    dev = gpu_device
    s = scene(S)
    vertices, masks, depths = on_device(s, dev)
    V = len(s.vertices)
    # through the entry point itself, into arrays full of garbage: every row is written
    table = (_lib.GsrCullView * max(S, 1))()
    for k, cam in enumerate(s.cameras):
        H, W, fx, fy = R.focal(cam)
        row = table[k]
        row.width, row.height, row.fx, row.fy = W, H, float(fx), float(fy)
        row.world_to_view[:] = cam.world_view_transform.reshape(-1).tolist()
        row.mask = None if masks[k] is None else masks[k].data_ptr()
        row.depth = None if depths[k] is None else depths[k].data_ptr()
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    in_view, visible = garbage(V, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.load().gsr_cull_view_counts(vertices.data_ptr(), V, table_dev.data_ptr() if S else None, S, s.near,
                                                s.depth_tol, 0, in_view.data_ptr(), visible.data_ptr(), stream), "counts")
    want_in, want_vis, fragile = s.want
    got_in, got_vis = in_view.cpu().numpy(), visible.cpu().numpy()
    print(f"[mesh_cull] S={S}: {int(fragile.sum())} fragile of {V * S} pairs; in_view off on {int((got_in != want_in).sum())}, "
          f"visible off on {int((got_vis != want_vis).sum())} vertices")
    assert np.all(np.abs(got_in - want_in) <= fragile) and np.all(np.abs(got_vis - want_vis) <= fragile)
    assert np.all(got_in[fragile == 0] == want_in[fragile == 0]) and np.all(got_vis[fragile == 0] == want_vis[fragile == 0])
    if S == 0:
        assert not got_in.any() and not got_vis.any()
    else:
        assert got_vis.sum() > 0 and (got_vis <= got_in).all()
    # the Python function gives the same bits, and gives them again
    for _ in range(2):
        a, b = vertex_view_counts(vertices, s.cameras, masks=masks, depths=depths, near=s.near, depth_tol=s.depth_tol)
        assert a.dtype == b.dtype == torch.int32 and torch.equal(a, in_view) and torch.equal(b, visible)
    # ... and in two chunks, accumulated, from zeros and on top of what is there
    if S >= 2:
        cut = S // 3 + 1
        first = vertex_view_counts(vertices, s.cameras[:cut], masks=masks[:cut], depths=depths[:cut], near=s.near,
                                   depth_tol=s.depth_tol)
        both = vertex_view_counts(vertices, s.cameras[cut:], masks=masks[cut:], depths=depths[cut:], near=s.near,
                                  depth_tol=s.depth_tol, counts=first)
        assert both[0] is first[0] and both[1] is first[1]
        assert torch.equal(both[0], in_view) and torch.equal(both[1], visible)
    base = (torch.arange(V, dtype=torch.int32, device=dev), torch.full((V,), 5, dtype=torch.int32, device=dev))
    vertex_view_counts(vertices, s.cameras, masks=masks, depths=depths, near=s.near, depth_tol=s.depth_tol, counts=base)
    assert torch.equal(base[0], in_view + torch.arange(V, dtype=torch.int32, device=dev)) and torch.equal(base[1], visible + 5)


def test_dyadic_case_is_exact_everywhere(gpu_device):
    from mvs_gaussian_splatting_amd import vertex_view_counts
    d = R.dyadic()
    vertices, masks, depths = on_device(d, gpu_device)
    a, b = vertex_view_counts(vertices, d.cameras, masks=[None if m is None else m.bool() for m in masks], depths=depths,
                              near=d.near, depth_tol=d.depth_tol)
    want_in, want_vis, fragile = R.counts(d.vertices, d.cameras, d.masks, d.depths, d.near, d.depth_tol, dtype=np.float64)
    assert fragile.sum() > 0.1 * len(d.vertices)
    assert np.array_equal(a.cpu().numpy(), want_in) and np.array_equal(b.cpu().numpy(), want_vis)
    empty = vertex_view_counts(vertices[:0], d.cameras, masks=masks, depths=depths)
    assert tuple(empty[0].shape) == tuple(empty[1].shape) == (0,) and empty[0].dtype == torch.int32


@pytest.mark.parametrize("shape", [(37, 70), (1, 1)])
def test_dilation_is_the_restatements(gpu_device, shape):
    from mvs_gaussian_splatting_amd import dilate_mask
    rng = np.random.default_rng(3)
    mask = (rng.random(shape) < 0.04).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    if shape == (1, 1):
        mask[:] = 9
    mask[-1, -1] = 200                                                   # a set pixel in the last corner
    for m in (mask, np.zeros(shape, dtype=np.uint8)):
        dev_mask = torch.from_numpy(m).to(gpu_device)
        for r in (0, 1, 5, 64):
            got = dilate_mask(dev_mask, r)
            assert got.dtype == torch.uint8 and got.data_ptr() != dev_mask.data_ptr()
            assert np.array_equal(got.cpu().numpy(), R.dilate(m, r)), (shape, r)
            assert torch.equal(dilate_mask(dev_mask != 0, r), got), "a bool mask is the same mask"
        assert torch.equal(dev_mask.cpu(), torch.from_numpy(m)), "the input is not written"


def _bits(t):
    return t.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("min_views", [1, 2, "all"])
@pytest.mark.parametrize("with_colors", [True, False])
def test_culling_end_to_end_is_the_restatements(gpu_device, min_views, with_colors):
    from mvs_gaussian_splatting_amd import cull_mesh_by_views
    dev = gpu_device
    s = scene(5)
    vertices, masks, depths = on_device(s, dev)
    faces = torch.from_numpy(s.faces).to(dev)
    colors = torch.from_numpy(s.colors).to(dev) if with_colors else None
    out = cull_mesh_by_views(vertices, faces, colors, cameras=s.cameras, masks=masks, depths=depths, min_views=min_views,
                             near=s.near, depth_tol=s.depth_tol, return_counts=True)
    v, f, c, (in_view, visible) = out
    # the restatement's culling on the device's own counts (whose agreement with the restatement's is the test above)
    want_v, want_f, want_c, kept_v, kept_f = R.cull(s.vertices, s.faces, s.colors if with_colors else None,
                                                    in_view.cpu().numpy(), visible.cpu().numpy(), min_views)
    assert 0 < len(want_v) < len(s.vertices) and 0 < len(want_f) and (min_views == 1 or len(want_f) < len(s.faces))
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and tuple(v.shape) == (len(want_v), 3)
    assert np.array_equal(_bits(v), want_v.view(np.int32)), "kept vertex rows are bit-copies, in order"
    assert np.array_equal(f.cpu().numpy(), want_f), "kept faces are re-indexed, in order"
    assert (c is None) == (not with_colors) and (c is None or np.array_equal(_bits(c), want_c.view(np.int32)))
    assert not np.isnan(v.cpu().numpy()).any() and int(f.max()) == len(want_v) - 1
    plain = cull_mesh_by_views(vertices, faces, colors, cameras=s.cameras, masks=masks, depths=depths, min_views=min_views,
                               near=s.near, depth_tol=s.depth_tol)
    assert len(plain) == 3 and torch.equal(plain[0], v) and torch.equal(plain[1], f)


def test_culling_edges_dilation_and_refusals(gpu_device):
    from mvs_gaussian_splatting_amd import _lib, cull_mesh_by_views, vertex_view_counts
    dev = gpu_device
    s = scene(5)
    vertices, masks, depths = on_device(s, dev)
    faces, colors = torch.from_numpy(s.faces).to(dev), torch.from_numpy(s.colors).to(dev)
    referenced = np.unique(s.faces)
    # everything kept: min_views 0.  The unreferenced vertices go, as in clean_mesh
    v, f, c = cull_mesh_by_views(vertices, faces, colors, cameras=s.cameras, min_views=0)
    assert np.array_equal(_bits(v), s.vertices[referenced].view(np.int32)) and np.array_equal(_bits(c), s.colors[referenced].view(np.int32))
    assert np.array_equal(referenced[f.cpu().numpy()], s.faces)
    # nothing kept: more views asked for than there are; and no cameras at all
    for cams, kw in ((s.cameras, {"min_views": 6}), ([], {}), ([], {"min_views": "all", "counts": (
            torch.ones(len(s.vertices), dtype=torch.int32, device=dev), torch.zeros(len(s.vertices), dtype=torch.int32, device=dev))})):
        v, f, c = cull_mesh_by_views(vertices, faces, colors, cameras=cams, **kw)
        assert tuple(v.shape) == tuple(f.shape) == tuple(c.shape) == (0, 3) and f.dtype == torch.int32 and v.device == vertices.device
    assert cull_mesh_by_views(vertices, faces, cameras=s.cameras, min_views=6)[2] is None
    # F == 0
    v, f, c, counts = cull_mesh_by_views(vertices, faces[:0], colors, cameras=s.cameras, return_counts=True)
    assert tuple(v.shape) == tuple(f.shape) == tuple(c.shape) == (0, 3) and tuple(counts[0].shape) == (len(s.vertices),)
    # dilate=r is the dilation of every mask first; counts= stands for the views already counted
    in_masks = [None if m is None else torch.from_numpy(R.sphere_maps(cam)[0]).to(dev) for cam, m in zip(s.cameras, s.masks)]
    got = cull_mesh_by_views(vertices, faces, colors, cameras=s.cameras, masks=in_masks, min_views="all", dilate=2,
                             near=s.near, depth_tol=s.depth_tol)
    want = cull_mesh_by_views(vertices, faces, colors, cameras=s.cameras, masks=masks, min_views="all", near=s.near,
                              depth_tol=s.depth_tol)
    tight = cull_mesh_by_views(vertices, faces, colors, cameras=s.cameras, masks=in_masks, min_views="all", near=s.near,
                               depth_tol=s.depth_tol)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and len(tight[1]) <= len(want[1])
    counts = vertex_view_counts(vertices, s.cameras[:2], masks=masks[:2], near=s.near, depth_tol=s.depth_tol)
    chunked = cull_mesh_by_views(vertices, faces, colors, cameras=s.cameras[2:], masks=masks[2:], min_views="all",
                                 near=s.near, depth_tol=s.depth_tol, counts=counts)
    assert all(torch.equal(a, b) for a, b in zip(chunked, want))
    in_view, visible = cull_mesh_by_views(vertices, faces, cameras=s.cameras, masks=masks, min_views="all", near=s.near,
                                          depth_tol=s.depth_tol, return_counts=True)[3]
    kept_v = R.cull(s.vertices, s.faces, None, in_view.cpu().numpy(), visible.cpu().numpy(), "all")[3]
    assert len(kept_v) == len(want[0]) and not (s.part[kept_v] == R.FLOATER).any() and (s.part[kept_v] == R.SPHERE).any()
    # a face index out of range
    for bad in (len(s.vertices), -1):
        broken = faces.clone()
        broken[7, 1] = bad
        with pytest.raises(_lib.GsrError, match="outside 0"):
            cull_mesh_by_views(vertices, broken, colors, cameras=s.cameras, min_views=0)


def test_clean_mesh_still_compacts_as_the_culling_does(gpu_device):
    """The tail the two share: with every face kept, both are the compaction of the referenced vertices."""
    from mvs_gaussian_splatting_amd import clean_mesh, cull_mesh_by_views
    s = scene(5)
    vertices, faces = torch.from_numpy(s.vertices).to(gpu_device), torch.from_numpy(s.faces).to(gpu_device)
    a = clean_mesh(vertices, faces, min_faces=0)
    b = cull_mesh_by_views(vertices, faces, cameras=[], min_views=0)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and a[2] is None and b[2] is None


def test_view_counts_for_views_is_chunk_independent(gpu_device):
    from mvs_gaussian_splatting_amd import TSDFVolume, fuse_views, vertex_view_counts, view_counts_for_views
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from mvs_gaussian_splatting_amd.tsdf import render_surface
    from mvs_gaussian_splatting_amd.renderer import render
    dev = gpu_device
    model, cam0, bg, _ = small_scene(scale=0.08)
    cameras = [cam0.to(dev)] + [small_scene(P=1, view=v)[1].to(dev) for v in (1, 3)]
    model.to(dev)
    bg, pipe = bg.to(dev), PipelineParams()
    volume = fuse_views(cameras, model, pipe, bg, TSDFVolume((-2.0, -1.5, 3.0), 0.125, (33, 25, 41), 0.5, device=dev),
                        alpha_min=0.5, max_depth=7.5)
    vertices, faces, _ = volume.extract_mesh()
    assert len(vertices) > 500
    one = view_counts_for_views(cameras, model, pipe, bg, vertices, chunk=1, depth_tol=0.05)
    three = view_counts_for_views(cameras, model, pipe, bg, vertices, chunk=3, depth_tol=0.05)
    assert torch.equal(one[0], three[0]) and torch.equal(one[1], three[1])
    with torch.no_grad():
        depths = [render_surface(render, cam, model, pipe, bg, 0.5, 0.0)[0] for cam in cameras]
    by_hand = vertex_view_counts(vertices, cameras, depths=depths, depth_tol=0.05)
    assert torch.equal(one[0], by_hand[0]) and torch.equal(one[1], by_hand[1])
    frames = view_counts_for_views(cameras, model, pipe, bg, vertices, occlusion=False, chunk=2)
    assert torch.equal(frames[0], one[0]) and torch.equal(frames[1], frames[0]), "without maps every view that holds it sees it"
    print(f"[mesh_cull] small scene: {int((one[1] > 0).sum())} of {len(vertices)} vertices visible somewhere, "
          f"{int((one[0] > 0).sum())} inside some image")
    assert int((one[1] > 0).sum()) >= 1 and bool((one[1] <= one[0]).all()) and int(one[0].max()) <= 3
