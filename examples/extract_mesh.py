"""From a trained model to a triangle mesh: render depth from the training views, fuse it into a TSDF volume and extract
the surface by marching tetrahedra, all on the HIP path (``mvs_gaussian_splatting_amd/tsdf.py``).

    python examples/extract_mesh.py -m <model directory> [--iteration N] [--voxel_size S | --resolution R]
                                    [--sdf_trunc T] [--alpha_min A] [--max_depth D] [--depth_ratio R]
                                    [--num_cluster N] [--min_cluster_faces M] [--unbounded [--mesh_res N]]
                                    [--consistent K] [--n_sources S] [--points] [--unbiased_depth]
                                    [--simplify_voxel S] [--cull_views K|all] [--cull_masks DIR] [--cull_dilate R]
                                    [--cull_occluded TOL] [--cull_invisible K] [-s <dataset>] [-r ...]

The scene is loaded as ``examples/render.py`` loads it (``cfg_args.json`` of the model directory; ``-s`` and the other
switches override it).  The volume bounds the bulk of the model's positions (``tsdf.volume_for_points``); ``--resolution``
is the number of samples along its longest side (default 256), ``--sdf_trunc`` defaults to 4 voxels.  Every training
view contributes its expected depth ``depth / alpha`` where ``alpha >= --alpha_min``; with ``--depth_ratio R`` (in [0, 1])
the blend ``(1 - R) expected + R median`` depth (``surface_depth``): 2DGS meshes bounded scenes at 1, where a pixel that sees
a thin edge in front of a far wall lands on one of the two instead of between them.

writes ``<model>/mesh/iteration_<N>/tsdf_mesh.ply`` (binary PLY, vertex colours from the renders).  With ``--num_cluster N``
and / or ``--min_cluster_faces M`` (50 when only ``--num_cluster`` is given; 2DGS: 50 and 50) the mesh is cleaned as 2DGS
cleans it -- the connected triangles are clustered and the clusters at least as large as the N-th largest, and of at
least M faces, are kept (``mesh.clean_mesh``) -- and written next to the raw one as ``tsdf_mesh_post.ply``.

``--unbounded`` meshes an unbounded scene as 2DGS's ``extract_mesh_unbounded`` does: the sphere of the
training cameras (``tsdf.bounding_sphere``) normalises the scene, the volume is a cube of contracted space with
``--mesh_res`` samples per side (default 512) that holds 95 % of the model (``tsdf.contracted_volume_for_points``), the
truncation is 5 voxels of the unit ball and grows with the distance (``--sdf_trunc`` overrides it), and the vertices go
back through the inverse contraction.  The mesh is written as ``tsdf_mesh_unbounded.ply``, the cleaned one as
``tsdf_mesh_unbounded_post.ply``; ``--voxel_size`` and ``--resolution`` belong to the bounded path.

``--consistent K`` filters every view's depth by multi-view geometric consistency before it is fused (``mvs.py``; DESIGN.md
§7.21): a pixel is integrated only if at least K of the view's ``--n_sources`` (default 4) nearest source views see it
where and as deep as it does, so floaters and depth that hangs between two surfaces never reach the volume.  ``--points``
also writes ``fused_points.ply`` next to the mesh: the fused point cloud of ``mvs.fuse_depth_points`` (xyz and 8-bit
colour; K defaults to 2 there), the product DTU-style evaluation is defined on.  Without these flags the output is unchanged.

``--unbiased_depth`` fuses PGSR's unbiased depth (``fuse_views(unbiased_depth=True)``) where the expected
depth stood: the depth at which each pixel's ray meets the blended plane of the Gaussians it sees, which lies on a slanted
surface where the expected depth bends towards the camera.  ``--depth_ratio`` blends the median into it as before.

``--simplify_voxel S`` makes the mesh smaller by vertex clustering on a grid of cells of S world units (``mesh.simplify_mesh``;
DESIGN.md §7.26): the vertices of a cell become their mean, the faces that collapse or repeat go.  It runs on the cleaned
mesh when the mesh is cleaned, else on the raw one, and writes ``tsdf_mesh_simplified.ply`` (``tsdf_mesh_unbounded_simplified.ply``)
next to the others.  A cell of two or three TSDF voxels suits a marching-tetrahedra mesh.  Without the flag nothing changes.

``--cull_views K|all``, ``--cull_masks DIR`` and ``--cull_occluded TOL`` cull the mesh by the training views
(``mesh.cull_mesh_by_views``), after the cleaning and before the simplification, and write
``tsdf_mesh_culled.ply`` (``tsdf_mesh_unbounded_culled.ply``) next to the others.  Every vertex is projected into every
training view; a view sees it when it lands inside the image, on the object mask if there are masks
(``DIR/<image_name>.png``, non-zero is object, resized with nearest to the camera's size; ``--cull_dilate R`` dilates them
by R pixels first, 2DGS: 25), and, with ``--cull_occluded TOL``, not more than TOL (relative) behind the surface the view
itself renders.  A vertex stays when K views see it; ``all``: every view whose image holds it, DTU's rule, the default
with masks (1 without).  Faces with a dropped corner go.  Without these flags nothing changes.

``--cull_invisible K`` then removes the faces that fewer than K training views see in the mesh's own z-buffer
(``mesh.cull_invisible_faces``): inner walls, shells inside closed objects and the back of the truncation
band, which a vertex test within a depth tolerance keeps.  It runs after the view culling and before the simplification and
writes ``tsdf_mesh_visible.ply`` (``tsdf_mesh_unbounded_visible.ply``).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvs_gaussian_splatting_amd import (GaussianModel, ModelParams, Scene, bounding_sphere,  # noqa: E402
                                        contracted_volume_for_points, fuse_depth_points, fuse_views,
                                        view_counts_for_views, volume_for_points)
from mvs_gaussian_splatting_amd.mesh import (clean_mesh, cull_invisible_faces, cull_mesh_by_views, dilate_mask,  # noqa: E402
                                             simplify_mesh)
from mvs_gaussian_splatting_amd.ply_io import write_ply_mesh, write_ply_vertices  # noqa: E402
from mvs_gaussian_splatting_amd.synthetic import PipelineParams  # noqa: E402


def write_points(path, xyz, rgb):
    """A point cloud as binary PLY: float x, y, z and uchar red, green, blue (colours clamped to [0, 1], times 255, rounded)."""
    xyz = xyz.detach().cpu().numpy()
    rgb = np.rint(np.clip(rgb.detach().cpu().numpy(), 0.0, 1.0) * 255.0).astype(np.uint8)
    elements = np.empty(xyz.shape[0], dtype=[("x", "f4"), ("y", "f4"), ("z", "f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for c, name in enumerate(("x", "y", "z")):
        elements[name] = xyz[:, c]
    for c, name in enumerate(("red", "green", "blue")):
        elements[name] = rgb[:, c]
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    write_ply_vertices(path, elements)


def read_mask(folder, camera):
    """``folder/<image_name>.png`` as a uint8 [H,W] tensor on the GPU: non-zero (in any channel) is object; a mask of
    another size is resized with nearest to the camera's."""
    from PIL import Image
    image = Image.open(os.path.join(folder, camera.image_name + ".png"))
    size = (int(camera.image_width), int(camera.image_height))
    if image.size != size:
        image = image.resize(size, Image.NEAREST)
    pixels = np.asarray(image)
    if pixels.ndim == 3:
        pixels = pixels.any(axis=2)
    return torch.from_numpy(np.ascontiguousarray(pixels != 0).astype(np.uint8)).to("cuda")


def extract(dataset, iteration, voxel_size=None, resolution=None, sdf_trunc=None, alpha_min=0.5, max_depth=None,
            depth_ratio=0.0, num_cluster=None, min_cluster_faces=None, unbounded=False, mesh_res=None, consistent=None,
            n_sources=4, points=False, unbiased_depth=False, simplify_voxel=None, cull_views=None, cull_masks=None,
            cull_dilate=0, cull_occluded=None, cull_invisible=None):
    with torch.no_grad():
        gaussians = GaussianModel(dataset.sh_degree)
        scene = Scene(dataset, gaussians, load_iteration=iteration, shuffle=False)
        bg_color = [1, 1, 1] if dataset.white_background else [0, 0, 0]
        background = torch.tensor(bg_color, dtype=torch.float32, device="cuda")
        if unbounded:
            center, radius = bounding_sphere(scene.getTrainCameras())
            print(f"bounding sphere of the training cameras: center ({center[0]:.5g}, {center[1]:.5g}, {center[2]:.5g}), "
                  f"radius {radius:.5g}")
            volume = contracted_volume_for_points(gaussians.get_xyz, center, radius,
                                                  resolution=512 if mesh_res is None else mesh_res, sdf_trunc=sdf_trunc)
        else:
            volume = volume_for_points(gaussians.get_xyz, voxel_size=voxel_size, resolution=resolution, sdf_trunc=sdf_trunc)
        print(f"volume {volume.dims[0]} x {volume.dims[1]} x {volume.dims[2]}, voxel {volume.voxel_size:.5g}, "
              f"truncation {volume.sdf_trunc:.5g}")
        fuse_views(scene.getTrainCameras(), gaussians, PipelineParams(), background, volume, alpha_min=alpha_min,
                   max_depth=max_depth, **({"depth_ratio": depth_ratio} if depth_ratio else {}),
                   **({} if consistent is None else {"consistency": {"n_sources": n_sources, "min_views": consistent}}),
                   **({"unbiased_depth": True} if unbiased_depth else {}))
        vertices, faces, colors = volume.extract_mesh()
    path = os.path.join(dataset.model_path, "mesh", "iteration_{}".format(scene.loaded_iter),
                        "tsdf_mesh_unbounded.ply" if unbounded else "tsdf_mesh.ply")
    write_ply_mesh(path, vertices, faces, colors)
    print(f"{vertices.shape[0]} vertices, {faces.shape[0]} faces -> {path}")
    if points:
        xyz, rgb = fuse_depth_points(scene.getTrainCameras(), gaussians, PipelineParams(), background, n_sources=n_sources,
                                     min_views=2 if consistent is None else consistent, alpha_min=alpha_min,
                                     depth_ratio=depth_ratio)
        cloud = os.path.join(os.path.dirname(path), "fused_points.ply")
        write_points(cloud, xyz, rgb)
        print(f"{xyz.shape[0]} fused points -> {cloud}")
    if num_cluster is not None or min_cluster_faces is not None:
        if min_cluster_faces is None:
            min_cluster_faces = 50
        kept_v, kept_f, kept_c = clean_mesh(vertices, faces, colors, keep_largest=num_cluster, min_faces=min_cluster_faces)
        post = path[:-len(".ply")] + "_post.ply"
        write_ply_mesh(post, kept_v, kept_f, kept_c)
        print(f"cleaned (num_cluster {num_cluster}, min_cluster_faces {min_cluster_faces}): {kept_v.shape[0]} of "
              f"{vertices.shape[0]} vertices, {kept_f.shape[0]} of {faces.shape[0]} faces -> {post}")
        vertices, faces, colors = kept_v, kept_f, kept_c
    if cull_views is not None or cull_masks is not None or cull_occluded is not None:
        cameras = scene.getTrainCameras()
        masks = None if cull_masks is None else [read_mask(cull_masks, camera) for camera in cameras]
        if masks is not None and cull_dilate:
            masks = [dilate_mask(mask, cull_dilate) for mask in masks]
        if cull_views is None:
            cull_views = 1 if masks is None else "all"
        counts = view_counts_for_views(cameras, gaussians, PipelineParams(), background, vertices, masks=masks,
                                       occlusion=cull_occluded is not None, alpha_min=alpha_min,
                                       **({"depth_ratio": depth_ratio} if depth_ratio else {}),
                                       **({"unbiased_depth": True} if unbiased_depth else {}),
                                       **({} if cull_occluded is None else {"depth_tol": cull_occluded}))
        seen_v, seen_f, seen_c = cull_mesh_by_views(vertices, faces, colors, cameras=[], counts=counts, min_views=cull_views)
        culled = path[:-len(".ply")] + "_culled.ply"
        write_ply_mesh(culled, seen_v, seen_f, seen_c)
        print(f"culled by {len(cameras)} views (cull_views {cull_views}, masks {cull_masks}, dilate {cull_dilate}, "
              f"occluded {cull_occluded}): {seen_v.shape[0]} of {vertices.shape[0]} vertices, {seen_f.shape[0]} of "
              f"{faces.shape[0]} faces -> {culled}")
        vertices, faces, colors = seen_v, seen_f, seen_c
    if cull_invisible is not None:
        cameras = scene.getTrainCameras()
        seen_v, seen_f, seen_c = cull_invisible_faces(vertices, faces, colors, cameras=cameras, min_views=cull_invisible)
        visible = path[:-len(".ply")] + "_visible.ply"
        write_ply_mesh(visible, seen_v, seen_f, seen_c)
        print(f"faces seen by at least {cull_invisible} of {len(cameras)} views: {seen_f.shape[0]} of {faces.shape[0]} faces, "
              f"{seen_v.shape[0]} of {vertices.shape[0]} vertices -> {visible}")
        vertices, faces, colors = seen_v, seen_f, seen_c
    if simplify_voxel is not None:
        small_v, small_f, small_c = simplify_mesh(vertices, faces, colors, voxel_size=simplify_voxel)
        simplified = path[:-len(".ply")] + "_simplified.ply"
        write_ply_mesh(simplified, small_v, small_f, small_c)
        print(f"simplified (cells of {simplify_voxel:.5g}): {small_v.shape[0]} of {vertices.shape[0]} vertices, "
              f"{small_f.shape[0]} of {faces.shape[0]} faces -> {simplified}")
    return path


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-s", "--source_path", default=None)
    ap.add_argument("-m", "--model_path", required=True)
    ap.add_argument("--images", default=None)
    ap.add_argument("-r", "--resolution_scale", dest="image_resolution", type=int, default=None,
                    help="the dataset's image down-scaling (examples/render.py -r)")
    ap.add_argument("--eval", action="store_true", default=None)
    ap.add_argument("--white_background", action="store_true", default=None)
    ap.add_argument("--iteration", type=int, default=-1)
    size = ap.add_mutually_exclusive_group()
    size.add_argument("--voxel_size", type=float, default=None)
    size.add_argument("--resolution", type=int, default=None, help="samples along the volume's longest side (256)")
    ap.add_argument("--sdf_trunc", type=float, default=None, help="truncation distance (4 voxels)")
    ap.add_argument("--alpha_min", type=float, default=0.5)
    ap.add_argument("--max_depth", type=float, default=None)
    ap.add_argument("--depth_ratio", type=float, default=0.0,
                    help="share of the median depth in the fused surface (2DGS: 0 unbounded, 1 bounded)")
    ap.add_argument("--num_cluster", type=int, default=None,
                    help="clean the mesh: keep the clusters at least as large as the N-th largest (2DGS: 50)")
    ap.add_argument("--min_cluster_faces", type=int, default=None,
                    help="clean the mesh: drop clusters of fewer faces (50 when --num_cluster is given)")
    ap.add_argument("--unbounded", action="store_true",
                    help="fuse in contracted space about the training cameras' sphere (2DGS's extract_mesh_unbounded)")
    ap.add_argument("--mesh_res", type=int, default=None, help="with --unbounded: samples per side of the contracted cube (512)")
    ap.add_argument("--consistent", type=int, default=None, metavar="K",
                    help="fuse only pixels that at least K source views confirm (multi-view geometric consistency)")
    ap.add_argument("--n_sources", type=int, default=4, help="source views per view for --consistent / --points (4)")
    ap.add_argument("--points", action="store_true", help="also write the fused point cloud fused_points.ply")
    ap.add_argument("--unbiased_depth", action="store_true",
                    help="fuse PGSR's unbiased plane depth instead of the expected depth")
    ap.add_argument("--simplify_voxel", type=float, default=None, metavar="S",
                    help="simplify the mesh by vertex clustering on cells of S world units (after the cleaning, if any)")
    ap.add_argument("--cull_views", default=None, metavar="K|all",
                    help="cull the mesh: keep the vertices that K training views see; all: every view whose image holds them")
    ap.add_argument("--cull_masks", default=None, metavar="DIR",
                    help="cull the mesh: a view sees a vertex only on its object mask DIR/<image_name>.png (non-zero)")
    ap.add_argument("--cull_dilate", type=int, default=0, metavar="R", help="dilate the masks by R pixels first (2DGS: 25)")
    ap.add_argument("--cull_occluded", type=float, default=None, metavar="TOL",
                    help="cull the mesh: a view sees a vertex only within TOL (relative) of the surface it renders")
    ap.add_argument("--cull_invisible", type=int, default=None, metavar="K",
                    help="drop the faces that fewer than K training views see in the mesh's own z-buffer")
    args = ap.parse_args(argv)
    if args.cull_invisible is not None and args.cull_invisible < 0:
        ap.error("--cull_invisible must not be negative")
    if args.cull_views is not None and args.cull_views != "all":
        if not args.cull_views.isdigit():
            ap.error("--cull_views must be a non-negative integer or all")
        args.cull_views = int(args.cull_views)
    if not 0 <= args.cull_dilate <= 1024:
        ap.error("--cull_dilate must lie in 0..1024")
    if args.cull_dilate and args.cull_masks is None:
        ap.error("--cull_dilate belongs to --cull_masks")
    if args.cull_masks is not None and not os.path.isdir(args.cull_masks):
        ap.error("--cull_masks must be a directory")
    if args.cull_occluded is not None and not 0 <= args.cull_occluded < float("inf"):
        ap.error("--cull_occluded must be finite and not negative")
    if args.simplify_voxel is not None and not 0 < args.simplify_voxel < float("inf"):
        ap.error("--simplify_voxel must be positive and finite")
    if args.consistent is not None and args.consistent < 0:
        ap.error("--consistent must not be negative")
    if not 1 <= args.n_sources <= 64:
        ap.error("--n_sources must lie in 1..64")
    if args.mesh_res is not None and not args.unbounded:
        ap.error("--mesh_res belongs to --unbounded")
    if args.mesh_res is not None and args.mesh_res < 2:
        ap.error("--mesh_res must be at least 2")
    if args.unbounded and (args.voxel_size is not None or args.resolution is not None):
        ap.error("--voxel_size and --resolution belong to the bounded path: give --mesh_res")
    if args.num_cluster is not None and args.num_cluster < 1:
        ap.error("--num_cluster must be positive")
    if args.min_cluster_faces is not None and args.min_cluster_faces < 0:
        ap.error("--min_cluster_faces must not be negative")
    fields = {}
    cfg = os.path.join(args.model_path, "cfg_args.json")
    if os.path.exists(cfg):
        with open(cfg) as f:
            fields = json.load(f)
    for k in ("source_path", "images", "eval", "white_background"):
        if getattr(args, k) is not None:
            fields[k] = getattr(args, k)
    if args.image_resolution is not None:
        fields["resolution"] = args.image_resolution
    if not fields.get("source_path"):
        ap.error("no cfg_args.json in the model directory: give the dataset with -s")
    dataset = ModelParams(model_path=args.model_path, **fields)
    print("Extracting a mesh from " + args.model_path)
    extract(dataset, args.iteration, args.voxel_size, args.resolution, args.sdf_trunc, args.alpha_min, args.max_depth,
            args.depth_ratio, **({} if args.num_cluster is None and args.min_cluster_faces is None else
                                 {"num_cluster": args.num_cluster, "min_cluster_faces": args.min_cluster_faces}),
            **({"unbounded": True, "mesh_res": args.mesh_res} if args.unbounded else {}),
            **({} if args.consistent is None and not args.points else
               {"consistent": args.consistent, "n_sources": args.n_sources, "points": args.points}),
            **({"unbiased_depth": True} if args.unbiased_depth else {}),
            **({} if args.simplify_voxel is None else {"simplify_voxel": args.simplify_voxel}),
            **({} if args.cull_views is None and args.cull_masks is None and args.cull_occluded is None else
               {"cull_views": args.cull_views, "cull_masks": args.cull_masks, "cull_dilate": args.cull_dilate,
                "cull_occluded": args.cull_occluded}),
            **({} if args.cull_invisible is None else {"cull_invisible": args.cull_invisible}))


if __name__ == "__main__":
    main()
