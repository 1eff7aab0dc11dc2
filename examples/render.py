"""The reference's ``render.py:24-49`` on this package: load the Gaussians a training run saved under ``model_path`` and
write every view of the scene as PNG.

    python examples/render.py -m <model directory> [--iteration N] [--skip_train] [--skip_test]
                              [-s <COLMAP or Blender directory>] [-r ...] [--eval] [--white_background] [--depth]
                              [--use_trained_exp] [--normals] [--depth_normals] [--distortion] [--median_depth] [--plane_depth]
                              [--point_cloud <.ply or .npz>]

The dataset's location and options come from the ``cfg_args.json`` that ``examples/train.py -s ... -m ...`` left in the
model directory; ``-s`` and the other switches override it.

writes ``<model>/<train|test>/ours_<N>/renders/%05d.png`` and ``.../gt/%05d.png``.  The 8-bit images come from
``metrics.to_uint8_hwc`` (torchvision's ``save_image`` rounding) on the device; Pillow only encodes the files.
``--depth`` also writes ``.../depth/%05d.png``: the expected depth ``depth / alpha`` of every pixel as a 16-bit
greyscale PNG, scaled so that 65535 is the view's largest value (0 where nothing was composited); the scale of each
view is listed in ``.../depth/scales.json`` (metres per step).
``--normals`` also writes ``.../normal/%05d.png``: the view-space normal map ``sum w n`` of ``render(return_normals=True)``
as ``normal * 0.5 + 0.5`` in 8 bits.
``--depth_normals`` also writes ``.../depth_normal/%05d.png``: the normals of the rendered depth surface,
``depth_to_normals(depth, alpha, ...)`` (``normal_consistency.py``), as ``depth_normal * 0.5 + 0.5`` in 8 bits -- the map
the consistency loss pulls ``--normals`` towards; pixels without a valid normal come out mid-grey.
``--median_depth`` also writes ``.../median_depth/%05d.png``: 2DGS's median depth (``render(return_median_depth=True)``)
as a 16-bit greyscale PNG scaled like ``--depth`` (``.../median_depth/scales.json``), and ``.../median_depth/%05d_id.npy``:
the int32 ``[H,W]`` map of the Gaussian that owns each pixel (-1: none).
``--plane_depth`` also writes ``.../plane_depth/%05d.png``: PGSR's unbiased depth (``render(return_plane_depth=True)``;
0 where the frame has no surface) as a 16-bit greyscale PNG scaled like ``--depth`` (``.../plane_depth/scales.json``).
``--mesh PLY`` also rasterizes that triangle mesh from every view (``rasterize_mesh``, ``face_normal_map``):
``.../mesh_depth/%05d.png``, its depth as a 16-bit greyscale PNG scaled like ``--depth`` (``.../mesh_depth/scales.json``; 0: no
surface), and ``.../mesh_normal/%05d.png``, its view-space face normals as colours, next to the renders.
``--point_cloud FILE`` renders that file in place of the iteration's ``point_cloud.ply``: a ``.ply``, or by its extension
the vector-quantised ``.npz`` that ``examples/compress.py`` writes (``GaussianModel.load_compressed``).
``--use_trained_exp`` renders every view that has one with the exposure saved in the iteration's ``exposure.json``
(``examples/train.py --train_exposure``); test views have none and are rendered as they are.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvs_gaussian_splatting_amd import (GaussianModel, ModelParams, Scene, depth_to_normals, render,  # noqa: E402
                                        to_uint8_hwc)
from mvs_gaussian_splatting_amd.synthetic import PipelineParams  # noqa: E402


def save_png(image, path):
    from PIL import Image
    Image.fromarray(to_uint8_hwc(image).cpu().numpy()).save(path)


def save_distortion_png(dist, path):
    """The distortion map as 16-bit greyscale scaled by its maximum; returns the value one step stands for."""
    import numpy as np
    from PIL import Image
    top = float(dist.max())
    step = top / 65535.0 if top > 0 else 1.0
    Image.fromarray(torch.round(dist[0] / step).clamp(0, 65535).cpu().numpy().astype(np.uint16)).save(path)
    return step


def save_median_png(median, median_id, path, id_path):
    """The median depth as 16-bit greyscale and the id map as ``.npy``; returns the depth one step stands for."""
    import numpy as np
    from PIL import Image
    top = float(median.max())
    step = top / 65535.0 if top > 0 else 1.0
    Image.fromarray(torch.round(median[0] / step).clamp(0, 65535).cpu().numpy().astype(np.uint16)).save(path)
    np.save(id_path, median_id.cpu().numpy())
    return step


def save_plane_depth_png(plane, path):
    """The unbiased plane depth as 16-bit greyscale; returns the depth one step stands for."""
    import numpy as np
    from PIL import Image
    top = float(plane.max())
    step = top / 65535.0 if top > 0 else 1.0
    Image.fromarray(torch.round(plane[0] / step).clamp(0, 65535).cpu().numpy().astype(np.uint16)).save(path)
    return step


def save_depth_png(depth, alpha, path):
    """``depth / alpha`` as 16-bit greyscale; returns the depth one step stands for."""
    import numpy as np
    from PIL import Image
    expected = torch.where(alpha > 0, depth / alpha.clamp_min(1e-12), torch.zeros_like(depth))[0]
    top = float(expected.max())
    step = top / 65535.0 if top > 0 else 1.0
    steps = torch.round(expected / step).clamp(0, 65535).cpu().numpy().astype(np.uint16)
    Image.fromarray(steps).save(path)
    return step


def save_mesh_pngs(mesh, view, depth_path, normal_path):
    """The mesh ``(vertices, faces)`` from ``view``: its depth as 16-bit greyscale (0: no surface) and its view-space face
    normals as colours; returns the depth one step stands for."""
    import numpy as np
    from PIL import Image
    from mvs_gaussian_splatting_amd import face_normal_map, rasterize_mesh
    depth, face_id = rasterize_mesh(mesh[0], mesh[1], view)
    top = float(depth.max())
    step = top / 65535.0 if top > 0 else 1.0
    Image.fromarray(torch.round(depth / step).clamp(0, 65535).cpu().numpy().astype(np.uint16)).save(depth_path)
    normal = face_normal_map(mesh[0], mesh[1], face_id, view)
    save_png(torch.where(face_id[None] >= 0, normal * 0.5 + 0.5, torch.zeros_like(normal)), normal_path)
    return step


def render_set(model_path, name, iteration, views, gaussians, pipeline, background, depth=False,
               use_trained_exp=False, normals=False, depth_normals=False, distortion=False, median_depth=False,
               plane_depth=False, mesh=None):
    render_path = os.path.join(model_path, name, "ours_{}".format(iteration), "renders")
    gts_path = os.path.join(model_path, name, "ours_{}".format(iteration), "gt")
    depth_path = os.path.join(model_path, name, "ours_{}".format(iteration), "depth")
    os.makedirs(render_path, exist_ok=True)
    os.makedirs(gts_path, exist_ok=True)
    scales = []
    if depth:
        os.makedirs(depth_path, exist_ok=True)
    normal_path = os.path.join(model_path, name, "ours_{}".format(iteration), "normal")
    if normals:
        os.makedirs(normal_path, exist_ok=True)
    depth_normal_path = os.path.join(model_path, name, "ours_{}".format(iteration), "depth_normal")
    if depth_normals:
        os.makedirs(depth_normal_path, exist_ok=True)
    distortion_path = os.path.join(model_path, name, "ours_{}".format(iteration), "distortion")
    dist_scales = []
    if distortion:
        os.makedirs(distortion_path, exist_ok=True)
    median_path = os.path.join(model_path, name, "ours_{}".format(iteration), "median_depth")
    median_scales = []
    if median_depth:
        os.makedirs(median_path, exist_ok=True)
    plane_path = os.path.join(model_path, name, "ours_{}".format(iteration), "plane_depth")
    plane_scales = []
    if plane_depth:
        os.makedirs(plane_path, exist_ok=True)
    mesh_depth_path = os.path.join(model_path, name, "ours_{}".format(iteration), "mesh_depth")
    mesh_normal_path = os.path.join(model_path, name, "ours_{}".format(iteration), "mesh_normal")
    mesh_scales = []
    if mesh is not None:
        os.makedirs(mesh_depth_path, exist_ok=True)
        os.makedirs(mesh_normal_path, exist_ok=True)
    for idx, view in enumerate(views):
        with_exp = use_trained_exp and view.image_name in (gaussians.pretrained_exposures or {})
        pkg = render(view, gaussians, pipeline, background, **({"return_depth": True} if depth or depth_normals else {}),
                     **({"use_trained_exp": True} if with_exp else {}), **({"return_normals": True} if normals else {}),
                     **({"return_distortion": True} if distortion else {}),
                     **({"return_median_depth": True} if median_depth else {}),
                     **({"return_plane_depth": True} if plane_depth else {}))
        rendering = pkg["render"]
        save_png(rendering, os.path.join(render_path, "{0:05d}".format(idx) + ".png"))
        save_png(view.original_image[0:3, :, :].to(rendering.device), os.path.join(gts_path, "{0:05d}".format(idx) + ".png"))
        if depth:
            scales.append(save_depth_png(pkg["depth"], pkg["alpha"], os.path.join(depth_path, "{0:05d}".format(idx) + ".png")))
        if normals:
            save_png(pkg["normal"] * 0.5 + 0.5, os.path.join(normal_path, "{0:05d}".format(idx) + ".png"))
        if depth_normals:
            dn = depth_to_normals(pkg["depth"], pkg["alpha"], math.tan(view.FoVx * 0.5), math.tan(view.FoVy * 0.5))
            save_png(dn * 0.5 + 0.5, os.path.join(depth_normal_path, "{0:05d}".format(idx) + ".png"))
        if distortion:
            dist_scales.append(save_distortion_png(pkg["distortion"],
                                                   os.path.join(distortion_path, "{0:05d}".format(idx) + ".png")))
        if median_depth:
            stem = os.path.join(median_path, "{0:05d}".format(idx))
            median_scales.append(save_median_png(pkg["median_depth"], pkg["median_id"], stem + ".png", stem + "_id.npy"))
        if plane_depth:
            plane_scales.append(save_plane_depth_png(pkg["plane_depth"],
                                                     os.path.join(plane_path, "{0:05d}".format(idx) + ".png")))
        if mesh is not None:
            mesh_scales.append(save_mesh_pngs(mesh, view, os.path.join(mesh_depth_path, "{0:05d}".format(idx) + ".png"),
                                              os.path.join(mesh_normal_path, "{0:05d}".format(idx) + ".png")))
    if mesh is not None:
        with open(os.path.join(mesh_depth_path, "scales.json"), "w") as f:
            json.dump(mesh_scales, f)
    if plane_depth:
        with open(os.path.join(plane_path, "scales.json"), "w") as f:
            json.dump(plane_scales, f)
    if median_depth:
        with open(os.path.join(median_path, "scales.json"), "w") as f:
            json.dump(median_scales, f)
    if depth:
        with open(os.path.join(depth_path, "scales.json"), "w") as f:
            json.dump(scales, f)
    if distortion:
        with open(os.path.join(distortion_path, "scales.json"), "w") as f:
            json.dump(dist_scales, f)


def render_sets(dataset, iteration, pipeline, skip_train=False, skip_test=False, depth=False, use_trained_exp=False,
                normals=False, depth_normals=False, distortion=False, median_depth=False, plane_depth=False, mesh=None,
                point_cloud=None, fuse_filter=False):
    with torch.no_grad():
        if mesh is not None:
            from mvs_gaussian_splatting_amd.ply_io import read_ply_mesh
            mesh_v, mesh_f, _ = read_ply_mesh(mesh)
            mesh = (torch.from_numpy(mesh_v).to("cuda"), torch.from_numpy(mesh_f).to("cuda"))
        gaussians = GaussianModel(dataset.sh_degree)
        scene = Scene(dataset, gaussians, load_iteration=iteration, shuffle=False)
        if point_cloud is not None:                              # this file instead of the iteration's point_cloud.ply
            (gaussians.load_compressed if point_cloud.endswith(".npz") else gaussians.load_ply)(point_cloud)
        # a filter_3D property in the PLY (examples/train.py --filter_3d) is on the model now and every frame below is drawn
        # through it
        if fuse_filter:
            if gaussians.filter_3D is None:
                raise SystemExit("--fuse_filter: the point cloud carries no filter_3D property")
            fused = os.path.join(dataset.model_path, "point_cloud", f"iteration_{scene.loaded_iter}", "point_cloud_fused.ply")
            gaussians.save_ply(fused, fuse_filter=True)
            print(f"wrote {fused}: a standard PLY with the 3D filter baked into scale_* and opacity")
        bg_color = [1, 1, 1] if dataset.white_background else [0, 0, 0]
        background = torch.tensor(bg_color, dtype=torch.float32, device="cuda")
        if use_trained_exp and gaussians.pretrained_exposures is None:
            raise FileNotFoundError("--use_trained_exp: the iteration's point-cloud directory has no exposure.json")
        if not skip_train:
            render_set(dataset.model_path, "train", scene.loaded_iter, scene.getTrainCameras(), gaussians, pipeline,
                       background, depth, use_trained_exp, normals, depth_normals, distortion, median_depth,
                       **({"plane_depth": True} if plane_depth else {}), **({} if mesh is None else {"mesh": mesh}))
        if not skip_test:
            render_set(dataset.model_path, "test", scene.loaded_iter, scene.getTestCameras(), gaussians, pipeline,
                       background, depth, use_trained_exp, normals, depth_normals, distortion, median_depth,
                       **({"plane_depth": True} if plane_depth else {}), **({} if mesh is None else {"mesh": mesh}))
    return scene


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-s", "--source_path", default=None)
    ap.add_argument("-m", "--model_path", required=True)
    ap.add_argument("--images", default=None)
    ap.add_argument("-r", "--resolution", type=int, default=None)
    ap.add_argument("--eval", action="store_true", default=None)
    ap.add_argument("--white_background", action="store_true", default=None)
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("--skip_train", action="store_true")
    ap.add_argument("--skip_test", action="store_true")
    ap.add_argument("--depth", action="store_true", help="also write depth / alpha of every view as a 16-bit PNG")
    ap.add_argument("--normals", action="store_true", help="also write the view-space normal map of every view as PNG")
    ap.add_argument("--depth_normals", action="store_true",
                    help="also write the normals of the rendered depth surface of every view as PNG")
    ap.add_argument("--distortion", action="store_true",
                    help="also write the depth-distortion map of every view as a 16-bit PNG scaled by its maximum")
    ap.add_argument("--median_depth", action="store_true",
                    help="also write the median depth of every view as a 16-bit PNG and the Gaussian id map as .npy")
    ap.add_argument("--plane_depth", action="store_true",
                    help="also write PGSR's unbiased plane depth of every view as a 16-bit PNG")
    ap.add_argument("--use_trained_exp", action="store_true", help="apply the saved per-image exposures")
    ap.add_argument("--mesh", default=None, metavar="PLY",
                    help="also rasterize this triangle mesh from every view: mesh_depth/ (16-bit) and mesh_normal/ PNGs")
    ap.add_argument("--point_cloud", default=None, metavar="FILE",
                    help="render this file instead of the iteration's point_cloud.ply: a .ply, or the .npz of "
                         "examples/compress.py (chosen by extension)")
    ap.add_argument("--fuse_filter", action="store_true",
                    help="also write point_cloud_fused.ply next to the point cloud: a standard PLY with the model's 3D "
                         "smoothing filter baked in, for viewers that know nothing of the filter_3D property")
    args = ap.parse_args(argv)
    fields = {}
    cfg = os.path.join(args.model_path, "cfg_args.json")
    if os.path.exists(cfg):
        with open(cfg) as f:
            fields = json.load(f)
    for k in ("source_path", "images", "resolution", "eval", "white_background"):
        if getattr(args, k) is not None:
            fields[k] = getattr(args, k)
    if not fields.get("source_path"):
        ap.error("no cfg_args.json in the model directory: give the dataset with -s")
    dataset = ModelParams(model_path=args.model_path, **fields)
    print("Rendering " + args.model_path)
    render_sets(dataset, args.iteration, PipelineParams(), args.skip_train, args.skip_test, args.depth,
                args.use_trained_exp, args.normals, args.depth_normals, args.distortion, args.median_depth,
                **({"plane_depth": True} if args.plane_depth else {}), **({} if args.mesh is None else {"mesh": args.mesh}),
                **({} if args.point_cloud is None else {"point_cloud": args.point_cloud}),
                **({"fuse_filter": True} if args.fuse_filter else {}))


if __name__ == "__main__":
    main()
