"""Scene readers of the reference's ingest layer (``scene/dataset_readers.py``, ``scene/colmap_loader.py``), host only:
COLMAP ``sparse/0/{cameras,images,points3D}`` in binary or text, Blender ``transforms_*.json``, and the
``x y z nx ny nz red green blue`` point-cloud PLY, built on ``ply_io`` (no ``plyfile``).

``CameraInfo`` and ``SceneInfo`` keep the reference's field names.  Two things differ, on purpose:

* ``CameraInfo.image`` is the opened (not yet decoded) Pillow image in both readers.  The reference's Blender reader
  composites every frame over the background in numpy while it reads; here the frame stays RGBA and the extra field
  ``composite_bg`` carries the background, so that ``scene.load_cam`` composites on the GPU
  (``image_ingest.load_image``).  ``decode_image`` gives the uint8 array either way.
* the text reader of ``cameras.txt`` takes every camera model the binary reader takes; the field-of-view rule then
  rejects what it cannot handle with an error that names the model (the reference's text reader asserts ``PINHOLE``).

Pillow opens and decodes the image files and is imported inside the functions that need it.
"""
from __future__ import annotations

import json
import os
import struct
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np

from . import ply_io
from .sh import SH2RGB
from .synthetic import focal2fov, get_world2view2

# COLMAP's camera models: id -> (name, number of parameters)
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}


class BasicPointCloud(NamedTuple):
    points: np.ndarray
    colors: np.ndarray
    normals: np.ndarray


class CameraInfo(NamedTuple):
    uid: int
    R: np.ndarray
    T: np.ndarray
    FovY: float
    FovX: float
    image: object
    image_path: str
    image_name: str
    width: int
    height: int
    composite_bg: Optional[np.ndarray] = None
    # the image's training mask (``masks=``): the PNG ``decode_mask`` reads, non-zero keeps the pixel; None for none
    mask_path: Optional[str] = None
    # upstream 3DGS's depth prior (``-d``): the 16-bit PNG of the image's inverse depth ("" for none) and its entry of
    # ``sparse/0/depth_params.json`` with ``med_scale`` added (None without the file or without an entry)
    depth_path: str = ""
    depth_params: Optional[dict] = None


class SceneInfo(NamedTuple):
    point_cloud: Optional[BasicPointCloud]
    train_cameras: list
    test_cameras: list
    nerf_normalization: dict
    ply_path: str


class ColmapCamera(NamedTuple):
    id: int
    model: str
    width: int
    height: int
    params: np.ndarray


class ColmapImage(NamedTuple):
    id: int
    qvec: np.ndarray
    tvec: np.ndarray
    camera_id: int
    name: str


def fov2focal(fov: float, pixels: float) -> float:
    import math
    return pixels / (2 * math.tan(fov / 2))


def qvec2rotmat(qvec) -> np.ndarray:
    """``scene/colmap_loader.py:43-53``: the rotation matrix of the quaternion (w, x, y, z)."""
    w, x, y, z = qvec[0], qvec[1], qvec[2], qvec[3]
    return np.array([
        [1 - 2 * y**2 - 2 * z**2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
        [2 * x * y + 2 * w * z, 1 - 2 * x**2 - 2 * z**2, 2 * y * z - 2 * w * x],
        [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x**2 - 2 * y**2]])


# ---- COLMAP files ---------------------------------------------------------------------------------------------------
def _unpack(fid, fmt: str):
    size = struct.calcsize("<" + fmt)
    data = fid.read(size)
    if len(data) != size:
        raise ValueError("unexpected end of COLMAP file")
    return struct.unpack("<" + fmt, data)


def _data_lines(path: str):
    with open(path, "r") as fid:
        lines = [line.strip() for line in fid]
    return lines


def read_intrinsics_binary(path: str) -> dict:
    cameras = {}
    with open(path, "rb") as fid:
        for _ in range(_unpack(fid, "Q")[0]):
            camera_id, model_id, width, height = _unpack(fid, "iiQQ")
            if model_id not in CAMERA_MODELS:
                raise ValueError(f"{path}: unknown COLMAP camera model id {model_id}")
            name, num_params = CAMERA_MODELS[model_id]
            cameras[camera_id] = ColmapCamera(camera_id, name, width, height, np.array(_unpack(fid, "d" * num_params)))
    return cameras


def read_intrinsics_text(path: str) -> dict:
    cameras = {}
    for line in _data_lines(path):
        if line and line[0] != "#":
            e = line.split()
            cameras[int(e[0])] = ColmapCamera(int(e[0]), e[1], int(e[2]), int(e[3]), np.array(tuple(map(float, e[4:]))))
    return cameras


def read_extrinsics_binary(path: str) -> dict:
    images = {}
    with open(path, "rb") as fid:
        for _ in range(_unpack(fid, "Q")[0]):
            props = _unpack(fid, "idddddddi")
            name = b""
            while True:
                ch = fid.read(1)
                if not ch:
                    raise ValueError(f"{path}: unterminated image name")
                if ch == b"\x00":
                    break
                name += ch
            fid.seek(24 * _unpack(fid, "Q")[0], os.SEEK_CUR)             # the 2D points (x, y, point3D id) are not used
            images[props[0]] = ColmapImage(props[0], np.array(props[1:5]), np.array(props[5:8]), props[8],
                                           name.decode("utf-8"))
    return images


def read_extrinsics_text(path: str) -> dict:
    images = {}
    lines = iter(_data_lines(path))
    for line in lines:
        if line and line[0] != "#":
            e = line.split()
            images[int(e[0])] = ColmapImage(int(e[0]), np.array(tuple(map(float, e[1:5]))),
                                            np.array(tuple(map(float, e[5:8]))), int(e[8]), e[9])
            next(lines, None)                                              # the line of 2D points that follows
    return images


def read_points3D_binary(path: str):
    with open(path, "rb") as fid:
        n = _unpack(fid, "Q")[0]
        xyzs, rgbs, errors = np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 1))
        for i in range(n):
            p = _unpack(fid, "QdddBBBd")
            xyzs[i], rgbs[i], errors[i] = p[1:4], p[4:7], p[7]
            fid.seek(8 * _unpack(fid, "Q")[0], os.SEEK_CUR)              # the track
    return xyzs, rgbs, errors


def read_points3D_text(path: str):
    rows = [line.split() for line in _data_lines(path) if line and line[0] != "#"]
    n = len(rows)
    xyzs, rgbs, errors = np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 1))
    for i, e in enumerate(rows):
        xyzs[i] = tuple(map(float, e[1:4]))
        rgbs[i] = tuple(map(int, e[4:7]))
        errors[i] = float(e[7])
    return xyzs, rgbs, errors


# ---- the point-cloud PLY (:107-130) -----------------------------------------------------------------------------------
PCD_DTYPE = [("x", "f4"), ("y", "f4"), ("z", "f4"), ("nx", "f4"), ("ny", "f4"), ("nz", "f4"),
             ("red", "u1"), ("green", "u1"), ("blue", "u1")]


def pcd_elements(xyz, rgb) -> np.ndarray:
    """The structured array ``storePly`` hands to ``plyfile``: float32 positions, zero normals, colours cast to uint8."""
    xyz, rgb = np.asarray(xyz), np.asarray(rgb)
    elements = np.empty(xyz.shape[0], dtype=PCD_DTYPE)
    attributes = np.concatenate((xyz, np.zeros_like(xyz), rgb), axis=1)
    for i, (name, _) in enumerate(PCD_DTYPE):
        elements[name] = attributes[:, i]
    return elements


def storePly(path: str, xyz, rgb) -> None:
    ply_io.write_ply_vertices(path, pcd_elements(xyz, rgb))


def fetchPly(path: str) -> BasicPointCloud:
    v, _ = ply_io.read_ply_vertices(path)
    positions = np.vstack([v["x"], v["y"], v["z"]]).T
    colors = np.vstack([v["red"], v["green"], v["blue"]]).T / 255.0
    normals = np.vstack([v["nx"], v["ny"], v["nz"]]).T
    return BasicPointCloud(points=positions, colors=colors, normals=normals)


# ---- scenes ---------------------------------------------------------------------------------------------------------
def getNerfppNorm(cam_info) -> dict:
    """``:45-66``: minus the mean camera centre, and 1.1 times the largest distance of a camera from it."""
    centers = [np.linalg.inv(get_world2view2(cam.R, cam.T))[:3, 3:4] for cam in cam_info]
    centers = np.hstack(centers)
    center = np.mean(centers, axis=1, keepdims=True)
    diagonal = np.max(np.linalg.norm(centers - center, axis=0, keepdims=True))
    return {"translate": -center.flatten(), "radius": diagonal * 1.1}


def colmap_fov(intr: ColmapCamera):
    """``:85-95``: (FovY, FovX) of an undistorted camera; any other model is an error."""
    if intr.model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL"):
        return focal2fov(intr.params[0], intr.height), focal2fov(intr.params[0], intr.width)
    if intr.model == "PINHOLE":
        return focal2fov(intr.params[1], intr.height), focal2fov(intr.params[0], intr.width)
    raise ValueError(f"COLMAP camera model {intr.model!r} is not handled: only undistorted datasets (PINHOLE, "
                     f"SIMPLE_PINHOLE or SIMPLE_RADIAL cameras) are supported")


def _open_image(path: str):
    from PIL import Image                                       # lazy: the package imports without Pillow
    return Image.open(path)


def read_depth_params(path: str) -> Optional[dict]:
    """``sparse/0/depth_params.json`` as upstream reads it: ``{image stem: {"scale": s, "offset": o}}``, every entry given
    ``med_scale``, the median of the positive scales (0 when none is positive).  None when the file is not there."""
    if not os.path.isfile(path):
        return None
    with open(path, "r") as f:
        params = json.load(f)
    scales = np.array([params[key]["scale"] for key in params], dtype=np.float64)
    med_scale = float(np.median(scales[scales > 0])) if (scales > 0).sum() else 0.0
    for key in params:
        params[key]["med_scale"] = med_scale
    return params


def _with_depth_priors(train_cams: list, depths_folder: str, depths_params: Optional[dict]) -> list:
    """The training cameras with ``depth_path = <folder>/<image stem>.png`` and their ``depth_params`` entry; a training
    camera without its PNG is an error."""
    out = []
    for c in train_cams:
        depth_path = os.path.join(depths_folder, c.image_name + ".png")
        if not os.path.isfile(depth_path):
            raise FileNotFoundError(f"depth prior of image {c.image_name!r} not found: {depth_path}")
        out.append(c._replace(depth_path=depth_path,
                              depth_params=None if depths_params is None else depths_params.get(c.image_name)))
    return out


def find_mask(masks_folder: str, cam: CameraInfo) -> Optional[str]:
    """The mask file of a camera: ``<folder>/<image_name>.png`` (the convention of ``examples/extract_mesh.py
    --cull_masks``), else ``<folder>/<image file name>.png`` (COLMAP's ``img.jpg.png``); None when neither is there."""
    for name in (cam.image_name, os.path.basename(cam.image_path)):
        path = os.path.join(masks_folder, name + ".png")
        if os.path.isfile(path):
            return path
    return None


def _with_masks(train_cams: list, masks_folder: str) -> list:
    """The training cameras with their ``mask_path``; a training camera without a mask file is an error."""
    out = []
    for c in train_cams:
        path = find_mask(masks_folder, c)
        if path is None:
            raise FileNotFoundError(f"mask of image {c.image_name!r} not found: neither {c.image_name}.png nor "
                                    f"{os.path.basename(c.image_path)}.png is in {masks_folder}")
        out.append(c._replace(mask_path=path))
    return out


def decode_mask(path: str) -> np.ndarray:
    """The ``[h, w]`` uint8 mask of a file, decoded with Pillow: 255 where the pixel is non-zero -- in any channel of a
    multi-channel file --, else 0.  Non-zero keeps the pixel, as in ``examples/extract_mesh.py``'s ``read_mask`` and in
    COLMAP; a 0 / 1 label image and a 0 / 255 one are the same mask."""
    from PIL import Image
    with Image.open(path) as image:
        if image.mode == "P":                               # palette indices are not values
            image = image.convert("RGBA")
        a = np.array(image)
    if a.ndim == 3:
        a = a.any(axis=2)
    if a.ndim != 2:
        raise ValueError(f"{path}: a mask must be an image, got an array of shape {a.shape}")
    return np.ascontiguousarray((a != 0).astype(np.uint8) * np.uint8(255))


def readColmapCameras(cam_extrinsics: dict, cam_intrinsics: dict, images_folder: str, open_image=_open_image) -> list:
    cam_infos = []
    for key in cam_extrinsics:
        extr = cam_extrinsics[key]
        intr = cam_intrinsics[extr.camera_id]
        R = np.transpose(qvec2rotmat(extr.qvec))
        T = np.array(extr.tvec)
        FovY, FovX = colmap_fov(intr)
        image_path = os.path.join(images_folder, os.path.basename(extr.name))
        image_name = os.path.basename(image_path).split(".")[0]
        cam_infos.append(CameraInfo(uid=intr.id, R=R, T=T, FovY=FovY, FovX=FovX, image=open_image(image_path),
                                    image_path=image_path, image_name=image_name, width=intr.width, height=intr.height))
    return cam_infos


def readColmapSceneInfo(path: str, images, eval: bool, llffhold: int = 8, depths: str = "", masks: str = "") -> SceneInfo:
    """``depths``: upstream's ``-d``, a folder under ``path`` with one 16-bit inverse-depth PNG per training image, aligned
    by ``sparse/0/depth_params.json`` when that file is there; test cameras of an ``eval`` split carry no prior.
    ``masks``: a folder, under ``path`` or absolute, with one mask PNG per training image (``find_mask``); test cameras
    carry none."""
    sparse = os.path.join(path, "sparse/0")
    try:
        cam_extrinsics = read_extrinsics_binary(os.path.join(sparse, "images.bin"))
        cam_intrinsics = read_intrinsics_binary(os.path.join(sparse, "cameras.bin"))
    except Exception:
        cam_extrinsics = read_extrinsics_text(os.path.join(sparse, "images.txt"))
        cam_intrinsics = read_intrinsics_text(os.path.join(sparse, "cameras.txt"))
    reading_dir = "images" if images is None else images
    unsorted = readColmapCameras(cam_extrinsics, cam_intrinsics, os.path.join(path, reading_dir))
    cam_infos = sorted(unsorted, key=lambda x: x.image_name)
    if eval:
        train_cam_infos = [c for idx, c in enumerate(cam_infos) if idx % llffhold != 0]
        test_cam_infos = [c for idx, c in enumerate(cam_infos) if idx % llffhold == 0]
    else:
        train_cam_infos, test_cam_infos = cam_infos, []
    if depths:
        train_cam_infos = _with_depth_priors(train_cam_infos, os.path.join(path, depths),
                                             read_depth_params(os.path.join(sparse, "depth_params.json")))
    if masks:
        train_cam_infos = _with_masks(train_cam_infos, os.path.join(path, masks))
    nerf_normalization = getNerfppNorm(train_cam_infos)
    ply_path = os.path.join(path, "sparse/0/points3D.ply")
    if not os.path.exists(ply_path):
        print("Converting point3d.bin to .ply, will happen only the first time you open the scene.")
        try:
            xyz, rgb, _ = read_points3D_binary(os.path.join(sparse, "points3D.bin"))
        except Exception:
            xyz, rgb, _ = read_points3D_text(os.path.join(sparse, "points3D.txt"))
        storePly(ply_path, xyz, rgb)
    try:
        pcd = fetchPly(ply_path)
    except Exception:
        pcd = None
    return SceneInfo(point_cloud=pcd, train_cameras=train_cam_infos, test_cameras=test_cam_infos,
                     nerf_normalization=nerf_normalization, ply_path=ply_path)


def readCamerasFromTransforms(path: str, transformsfile: str, white_background: bool, extension: str = ".png",
                              open_image=_open_image) -> list:
    """``:179-219``; the composite of ``:204-210`` is left to ``scene.load_cam`` (``composite_bg``)."""
    cam_infos = []
    with open(os.path.join(path, transformsfile)) as json_file:
        contents = json.load(json_file)
    fovx = contents["camera_angle_x"]
    for idx, frame in enumerate(contents["frames"]):
        cam_name = os.path.join(path, frame["file_path"] + extension)
        c2w = np.array(frame["transform_matrix"])
        c2w[:3, 1:3] *= -1                       # OpenGL / Blender axes (Y up, Z back) -> COLMAP (Y down, Z forward)
        w2c = np.linalg.inv(c2w)
        R = np.transpose(w2c[:3, :3])            # stored transposed, as the rasterizer's host expects
        T = w2c[:3, 3]
        image_path = os.path.join(path, cam_name)
        image = open_image(image_path)
        bg = np.array([1, 1, 1]) if white_background else np.array([0, 0, 0])
        fovy = focal2fov(fov2focal(fovx, image.size[0]), image.size[1])
        cam_infos.append(CameraInfo(uid=idx, R=R, T=T, FovY=fovy, FovX=fovx, image=image, image_path=image_path,
                                    image_name=Path(cam_name).stem, width=image.size[0], height=image.size[1],
                                    composite_bg=bg))
    return cam_infos


def readNerfSyntheticInfo(path: str, white_background: bool, eval: bool, extension: str = ".png",
                          depths: str = "", masks: str = "") -> SceneInfo:
    """``depths``: as in ``readColmapSceneInfo``; a Blender scene has no ``depth_params.json``, so the priors are raw.
    ``masks``: as in ``readColmapSceneInfo``; the alpha channel of the RGBA frames is not taken as a mask."""
    train_cam_infos = readCamerasFromTransforms(path, "transforms_train.json", white_background, extension)
    test_cam_infos = readCamerasFromTransforms(path, "transforms_test.json", white_background, extension)
    if not eval:
        train_cam_infos.extend(test_cam_infos)
        test_cam_infos = []
    if depths:
        train_cam_infos = _with_depth_priors(train_cam_infos, os.path.join(path, depths), None)
    if masks:
        train_cam_infos = _with_masks(train_cam_infos, os.path.join(path, masks))
    nerf_normalization = getNerfppNorm(train_cam_infos)
    ply_path = os.path.join(path, "points3d.ply")
    if not os.path.exists(ply_path):
        num_pts = 100_000                        # no COLMAP cloud: random points inside the synthetic scenes' bounds
        print(f"Generating random point cloud ({num_pts})...")
        xyz = np.random.random((num_pts, 3)) * 2.6 - 1.3
        shs = np.random.random((num_pts, 3)) / 255.0
        storePly(ply_path, xyz, SH2RGB(shs) * 255)
    try:
        pcd = fetchPly(ply_path)
    except Exception:
        pcd = None
    return SceneInfo(point_cloud=pcd, train_cameras=train_cam_infos, test_cameras=test_cam_infos,
                     nerf_normalization=nerf_normalization, ply_path=ply_path)


sceneLoadTypeCallbacks = {"Colmap": readColmapSceneInfo, "Blender": readNerfSyntheticInfo}


def decode_invdepth(path: str) -> np.ndarray:
    """The ``[h, w]`` float32 inverse depth of a prior's PNG, ``uint16 / 65536`` (upstream's ``cv2.imread(path, -1) /
    2**16``), decoded with Pillow.  Anything but a 16-bit single-channel image is a ``ValueError`` that names the file."""
    from PIL import Image
    with Image.open(path) as image:
        if not image.mode.startswith("I;16"):
            raise ValueError(f"{path}: a depth prior must be a 16-bit single-channel PNG, got image mode {image.mode!r}")
        a = np.array(image)
    if a.ndim != 2:
        raise ValueError(f"{path}: a depth prior must be a 16-bit single-channel PNG, got an array of shape {a.shape}")
    return a.astype(np.float32) / np.float32(65536.0)


def decode_image(cam_info: CameraInfo) -> np.ndarray:
    """The decoded ``[H, W, 3 or 4]`` uint8 array of a camera's image: RGBA when it is to be composited
    (``image.convert("RGBA")``, ``:204``), else the file's own RGB or RGBA pixels."""
    image = cam_info.image
    if cam_info.composite_bg is not None:
        return np.array(image.convert("RGBA"))
    if image.mode not in ("RGB", "RGBA"):
        raise ValueError(f"{cam_info.image_path}: image mode {image.mode!r} is not supported (RGB or RGBA needed: the "
                         f"loss takes a 3-channel target)")
    return np.array(image)
