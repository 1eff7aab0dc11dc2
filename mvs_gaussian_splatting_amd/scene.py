"""``Scene``, ``Camera`` and ``loadCam`` of the reference's ingest layer (``scene/__init__.py``, ``scene/cameras.py``,
``utils/camera_utils.py``): point the package at a COLMAP or Blender directory.

    dataset = ModelParams(source_path=..., model_path=..., resolution=-1)
    gaussians = GaussianModel(dataset.sh_degree)
    scene = Scene(dataset, gaussians)
    for camera in scene.getTrainCameras(): ...          # camera.original_image is the [3, H, W] float32 target

The readers are ``dataset_readers``; every image goes from its decoded bytes to the training target on the GPU
(``image_ingest.load_image``).  One thing differs from the reference on purpose: ``loadCam`` tests ``shape[1] == 4`` (the
image *height*) to find an alpha channel, so there an RGBA image's mask is applied only to images four pixels tall;
here the alpha channel of an RGBA image always multiplies the target, which is what ``Camera.__init__`` does with the
mask it is given.
"""
from __future__ import annotations

import json
import os
import random

import numpy as np
import torch

from . import image_ingest
from .exposure import load_exposures, save_exposures
from .dataset_readers import decode_image, decode_invdepth, decode_mask, fov2focal, sceneLoadTypeCallbacks
from .synthetic import get_projection_matrix, get_world2view2


class ModelParams:
    """``arguments/__init__.py:47-66`` defaults."""
    sh_degree = 3
    source_path = ""
    model_path = ""
    images = "images"
    depths = ""              # upstream 3DGS's -d: the folder of per-image inverse-depth PNGs under source_path; "" for none
    masks = ""               # the folder of per-image training masks (PNG, non-zero keeps), under source_path or absolute; "" for none
    resolution = -1
    white_background = False
    data_device = "cuda"
    eval = False
    grow_dir = False
    continous_dir = False
    grow_distance = False
    num_dirs = 128
    prob_notreinit = False
    symmetric_split = False
    split_notreinit = False
    learn_split_distance = False
    learn_split_scale = False

    def __init__(self, **overrides):
        for k, v in overrides.items():
            if not hasattr(type(self), k):
                raise TypeError(f"ModelParams has no field {k!r}")
            setattr(self, k, v)
        if self.source_path:
            self.source_path = os.path.abspath(self.source_path)


class Camera:
    """``scene/cameras.py:17-57``.  image: the finished ``[3, H, W]`` float32 target (``image_ingest.load_image`` has
    clamped and masked it already); gt_alpha_mask: a further ``[1, H, W]`` mask to multiply in, as the reference's
    constructor does.  The matrices live on ``device``, the target on ``data_device``.
    invdepthmap, depth_params: upstream 3DGS's depth prior (``scene/cameras.py``): the ``[1, H, W]`` (or ``[H, W]``) float32
    inverse depth already at the camera's resolution, and its ``depth_params.json`` entry ``{"scale", "offset",
    "med_scale"}`` or None.  Negatives are clamped to 0; with an entry whose ``scale`` lies outside ``[0.2, 5] med_scale``
    the prior is unreliable (``depth_reliable = False``, ``depth_mask`` zeros); ``invdepth * scale + offset`` is applied
    when ``scale > 0``.  Attributes: ``invdepthmap`` and ``depth_mask`` (``[1, H, W]`` float32 on ``data_device``) and
    ``depth_reliable``; without a map None, None and False.
    alpha_mask: the image's training mask (``dataset_readers.decode_mask``), a uint8 ``[h, w]`` array or
    tensor, 0 to 255, or a float one already in ``[0, 1]`` at the camera's size.  It is kept as the attribute ``alpha_mask``,
    ``[1, H, W]`` float32 in ``[0, 1]`` on ``data_device``, for the masked losses -- it is NOT multiplied into
    ``original_image``, which is what ``gt_alpha_mask`` does.  A uint8 mask of another size is resized to the camera's
    with ``mask_to_float``.  Without one the attribute is None."""

    def __init__(self, colmap_id, R, T, FoVx, FoVy, image, gt_alpha_mask, image_name, uid,
                 trans=np.array([0.0, 0.0, 0.0]), scale=1.0, data_device="cuda", device="cuda", *,
                 invdepthmap=None, depth_params=None, alpha_mask=None):
        self.uid = uid
        self.colmap_id = colmap_id
        self.R = R
        self.T = T
        self.FoVx = FoVx
        self.FoVy = FoVy
        self.image_name = image_name
        try:
            self.data_device = torch.device(data_device)
        except Exception as e:
            print(e)
            print(f"[Warning] Custom device {data_device} failed, fallback to default cuda device")
            self.data_device = torch.device("cuda")
        self.original_image = image.clamp(0.0, 1.0).to(self.data_device)
        self.image_width = self.original_image.shape[2]
        self.image_height = self.original_image.shape[1]
        if gt_alpha_mask is not None:
            self.original_image *= gt_alpha_mask.to(self.data_device)
        self.invdepthmap, self.depth_mask, self.depth_reliable = None, None, False
        if invdepthmap is not None:
            m = torch.as_tensor(invdepthmap, dtype=torch.float32).reshape(1, self.image_height, self.image_width)
            m = m.to(self.data_device).clamp(min=0.0)
            self.depth_mask = torch.ones_like(m)
            self.depth_reliable = True
            if depth_params is not None:
                if (depth_params["scale"] < 0.2 * depth_params["med_scale"]
                        or depth_params["scale"] > 5 * depth_params["med_scale"]):
                    self.depth_reliable = False
                    self.depth_mask = torch.zeros_like(m)
                if depth_params["scale"] > 0:
                    m = m * float(depth_params["scale"]) + float(depth_params["offset"])
            self.invdepthmap = m
        self.alpha_mask = None
        if alpha_mask is not None:
            self.alpha_mask = mask_to_float(alpha_mask, (self.image_width, self.image_height), self.data_device)
        self.zfar = 100.0
        self.znear = 0.01
        self.trans = trans
        self.scale = scale
        self.world_view_transform = torch.tensor(get_world2view2(R, T, trans, scale)).transpose(0, 1).to(device)
        self.projection_matrix = get_projection_matrix(znear=self.znear, zfar=self.zfar, fovX=self.FoVx,
                                                       fovY=self.FoVy).transpose(0, 1).to(device)
        self.full_proj_transform = (self.world_view_transform.unsqueeze(0)
                                    .bmm(self.projection_matrix.unsqueeze(0))).squeeze(0)
        self.camera_center = self.world_view_transform.inverse()[3, :3]


def mask_to_float(mask, size, device) -> torch.Tensor:
    """A training mask as ``[1, H, W]`` float32 in ``[0, 1]`` on ``device``; ``size`` is (width, height).  A uint8 ``[h, w]``
    mask (0 to 255) of another size is first resized with Pillow's 8-bit bicubic, the filter the photographs are resized
    with: ``image_ingest.resize_u8`` on a GPU, Pillow itself -- the same bytes -- when ``device`` is the host; then ``/ 255``
    and a clamp.  A floating-point mask must already have the size and is only clamped."""
    W, H = int(size[0]), int(size[1])
    device = torch.device(device)
    m = torch.as_tensor(mask)
    if m.dim() == 3 and 1 in (m.shape[0], m.shape[2]):
        m = m.reshape(m.shape[1], m.shape[2]) if m.shape[0] == 1 else m.reshape(m.shape[0], m.shape[1])
    if m.dim() != 2 or m.numel() == 0:
        raise ValueError(f"alpha_mask must be [h, w], got {tuple(torch.as_tensor(mask).shape)}")
    if m.dtype == torch.uint8:
        if tuple(m.shape) != (H, W):
            if device.type == "cuda":
                m = image_ingest.resize_u8(m.to(device)[:, :, None].contiguous(), (W, H))[:, :, 0]
            else:
                from PIL import Image                           # lazy: the package imports without Pillow
                m = torch.from_numpy(np.array(Image.fromarray(m.cpu().numpy()).resize((W, H), Image.BICUBIC)))
        # v / 255 from a table rounded on the host: the same float32 whichever device divides
        m = (torch.arange(256, dtype=torch.float32) / 255.0).to(device)[m.to(device).long()]
    elif m.dtype.is_floating_point:
        if tuple(m.shape) != (H, W):
            raise ValueError(f"a floating-point alpha_mask must be at the camera's size {H} x {W}, got {tuple(m.shape)}")
        m = m.to(device).to(torch.float32)
    else:
        raise TypeError(f"alpha_mask must be uint8 (0 to 255) or floating point (0 to 1), got {m.dtype}")
    return m.clamp(0.0, 1.0).reshape(1, H, W).contiguous()


class MiniCam:
    """``scene/cameras.py:59-70``."""

    def __init__(self, width, height, fovy, fovx, znear, zfar, world_view_transform, full_proj_transform):
        self.image_width = width
        self.image_height = height
        self.FoVy = fovy
        self.FoVx = fovx
        self.znear = znear
        self.zfar = zfar
        self.world_view_transform = world_view_transform
        self.full_proj_transform = full_proj_transform
        self.camera_center = torch.inverse(self.world_view_transform)[3][:3]


def so3_exp(rot: torch.Tensor) -> torch.Tensor:
    """Rodrigues: the rotation matrix of the axis-angle vector ``rot[3]``, ``I + a K + b K^2`` with ``K = [rot]_x``,
    ``a = sin(t)/t`` and ``b = (1 - cos t)/t^2 = (sin(t/2)/(t/2))^2 / 2``.  Below ``t^2 = 1e-6`` the two factors are their
    series in ``t^2``, so the map and its derivative are exact at zero (where the result is the identity bit for bit)."""
    t2 = (rot * rot).sum()
    small = t2 < 1e-6
    t = torch.sqrt(torch.where(small, torch.ones_like(t2), t2))      # the unused branch stays away from sqrt(0)
    half = 0.5 * t
    a = torch.where(small, 1.0 - t2 / 6.0 + t2 * t2 / 120.0, torch.sin(t) / t)
    b = torch.where(small, 0.5 - t2 / 24.0 + t2 * t2 / 720.0, 0.5 * (torch.sin(half) / half) ** 2)
    x, y, z = rot[0], rot[1], rot[2]
    o = torch.zeros_like(x)
    K = torch.stack([torch.stack([o, -z, y]), torch.stack([z, o, -x]), torch.stack([-y, x, o])])
    return torch.eye(3, dtype=rot.dtype, device=rot.device) + a * K + b * (K @ K)


def pose_transforms(world_view, projection, full_proj, rot_delta, trans_delta):
    """(world_view_transform, full_proj_transform, camera_center) of a camera whose world-to-camera transform is
    ``D @ W2C``, ``D = [[so3_exp(rot_delta), trans_delta], [0, 1]]``.  The tensors are the row-vector-convention ones of
    ``Camera`` (``world_view = W2C^T``), so the increment multiplies from the right: ``world_view @ D^T``; the other two
    follow with ``Camera``'s own ops (``bmm`` with the projection matrix, ``inverse()[3, :3]``).  A camera without a
    projection matrix (``MiniCam``; pass ``projection=None``) gets ``full_proj + world_view (D^T - I) inv(world_view)
    full_proj``: the same matrix, and again the base's bits at zero delta."""
    dR = so3_exp(rot_delta)
    zero = torch.zeros(3, 1, dtype=dR.dtype, device=dR.device)
    one = torch.ones(1, dtype=dR.dtype, device=dR.device)
    Dt = torch.cat([torch.cat([dR.transpose(0, 1), zero], dim=1), torch.cat([trans_delta, one]).unsqueeze(0)], dim=0)
    if not world_view.is_contiguous() and world_view.transpose(0, 1).is_contiguous():
        # Camera keeps its matrix as a transposed view; the product takes the same strides, so that inverse() and bmm
        # below walk the memory they walk for the base camera and give the same bits at zero delta
        view = (Dt.transpose(0, 1) @ world_view.transpose(0, 1)).transpose(0, 1)
    else:
        view = world_view @ Dt
    if projection is not None:
        full = (view.unsqueeze(0).bmm(projection.unsqueeze(0))).squeeze(0)
    else:
        eye = torch.eye(4, dtype=Dt.dtype, device=Dt.device)
        full = full_proj + world_view @ (Dt - eye) @ (world_view.inverse() @ full_proj)
    return view, full, view.inverse()[3, :3]


class PoseCamera(torch.nn.Module):
    """A camera with a learnable pose: wraps a ``Camera``, ``MiniCam`` or ``SyntheticCamera`` and applies the SE(3)
    increment (``rot_delta[3]`` axis-angle, ``trans_delta[3]``) on the left of its world-to-camera transform.

    ``world_view_transform``, ``full_proj_transform`` and ``camera_center`` are computed by torch on the base camera's
    device every time they are read and carry the graph back to the two parameters; ``render()`` hands them to the
    rasterizer, whose backward returns their gradients.  Every other attribute ``render()`` or the training loop reads
    (``image_width``, ``FoVx``, ``original_image``, ...) is the base camera's.  At zero delta the three tensors are
    ``torch.equal`` to the base's: the frame is the base camera's frame bit for bit.

        cam = PoseCamera(scene.getTrainCameras()[0])
        pose_opt = torch.optim.Adam(cam.parameters(), lr=1e-3)
        training_iteration(model, cam, opt, pipe, background, it, cameras_extent=extent, pose_optimizer=pose_opt)
    """

    def __init__(self, base_camera):
        super().__init__()
        if isinstance(base_camera, PoseCamera):
            raise TypeError("PoseCamera wraps a plain camera: bake() the inner one first")
        self.__dict__["_base"] = base_camera
        wv = base_camera.world_view_transform
        self.rot_delta = torch.nn.Parameter(torch.zeros(3, dtype=wv.dtype, device=wv.device))
        self.trans_delta = torch.nn.Parameter(torch.zeros(3, dtype=wv.dtype, device=wv.device))

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            base = self.__dict__.get("_base")
            # a failure inside one of the three properties must surface, not fall back to the base camera's fixed tensor
            if base is None or name.startswith("__") or name in ("world_view_transform", "full_proj_transform",
                                                                  "camera_center"):
                raise
            return getattr(base, name)

    @property
    def base_camera(self):
        return self.__dict__["_base"]

    def transforms(self):
        """The three tensors at the current pose, from one evaluation of the increment."""
        b = self.base_camera
        return pose_transforms(b.world_view_transform, getattr(b, "projection_matrix", None), b.full_proj_transform,
                               self.rot_delta, self.trans_delta)

    @property
    def world_view_transform(self):
        return self.transforms()[0]

    @property
    def full_proj_transform(self):
        return self.transforms()[1]

    @property
    def camera_center(self):
        return self.transforms()[2]

    def pose(self):
        """The current (R, T) in ``Camera``'s convention (R camera-to-world, T the world-to-camera translation), float64
        numpy, evaluated in float64 from the base camera's matrix and the two parameters."""
        with torch.no_grad():
            wv = self.base_camera.world_view_transform.detach().double().cpu()
            view, _, _ = pose_transforms(wv, None, wv, self.rot_delta.detach().double().cpu(),
                                         self.trans_delta.detach().double().cpu())
        return view[:3, :3].numpy().copy(), view[3, :3].numpy().copy()

    def bake(self):
        """A plain camera of the base's class at the current pose (for ``MiniCam``: the current matrices, detached)."""
        b = self.base_camera
        R, T = self.pose()
        if isinstance(b, Camera):
            dev = b.world_view_transform.device
            return Camera(b.colmap_id, R, T, b.FoVx, b.FoVy, b.original_image, None, b.image_name, b.uid,
                          data_device=b.data_device, device=dev, alpha_mask=getattr(b, "alpha_mask", None))
        if isinstance(b, MiniCam):
            with torch.no_grad():
                view, full, _ = self.transforms()
            return MiniCam(b.image_width, b.image_height, b.FoVy, b.FoVx, b.znear, b.zfar, view.detach(), full.detach())
        from .synthetic import SyntheticCamera
        if isinstance(b, SyntheticCamera):
            return SyntheticCamera(b.image_width, b.image_height, fov2focal(b.FoVx, b.image_width),
                                   fov2focal(b.FoVy, b.image_height), R=R, T=T, znear=b.znear, zfar=b.zfar,
                                   device=b.world_view_transform.device)
        raise TypeError(f"cannot bake a {type(b).__name__}: PoseCamera knows Camera, MiniCam and SyntheticCamera")


_WARNED = False


def load_resolution(orig_w: int, orig_h: int, resolution, resolution_scale: float = 1.0):
    """``loadCam``'s (width, height) (``utils/camera_utils.py:20-39``): ``-r`` 1/2/4/8 divides and rounds with Python's
    ``round``; -1 scales images wider than 1600 pixels down to 1600; any other value is the target width; those two
    truncate with ``int``."""
    global _WARNED
    if resolution in [1, 2, 4, 8]:
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        if orig_w > 1600:
            if not _WARNED:
                print("[ INFO ] Encountered quite large input images (>1.6K pixels width), rescaling to 1.6K.\n "
                      "If this is not desired, please explicitly specify '--resolution/-r' as 1")
                _WARNED = True
            global_down = orig_w / 1600
        else:
            global_down = 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


def load_invdepth(path: str, resolution, device="cuda") -> torch.Tensor:
    """The prior of ``path`` (``dataset_readers.decode_invdepth``: ``uint16 / 65536``) as ``[1, H, W]`` float32 on ``device``
    at ``resolution = (W, H)``: resized with ``interpolate(mode="bilinear", align_corners=False, antialias=False)``, the
    sampling rule of ``cv2.INTER_LINEAR`` that upstream resizes with (not claimed bit-equal to OpenCV's fixed-point
    arithmetic).  Once per image, at load."""
    m = torch.from_numpy(decode_invdepth(path)).to(device)[None, None]
    W, H = int(resolution[0]), int(resolution[1])
    if tuple(m.shape[-2:]) != (H, W):
        m = torch.nn.functional.interpolate(m, size=(H, W), mode="bilinear", align_corners=False, antialias=False)
    return m[0]


def load_cam(args, id, cam_info, resolution_scale, device="cuda") -> Camera:
    """``loadCam``: decode on the host, then composite / resize / convert on ``device``.  A camera whose ``CameraInfo``
    names a depth prior gets it through ``load_invdepth``, one that names a mask gets ``decode_mask``'s array as its
    ``alpha_mask``; any other camera is built by the calls made before priors and masks."""
    orig_w, orig_h = cam_info.image.size
    resolution = load_resolution(orig_w, orig_h, args.resolution, resolution_scale)
    target = image_ingest.load_image(decode_image(cam_info), resolution, device, composite_bg=cam_info.composite_bg)
    prior = {}
    if getattr(cam_info, "depth_path", ""):
        prior = {"invdepthmap": load_invdepth(cam_info.depth_path, resolution, device),
                 "depth_params": cam_info.depth_params}
    if getattr(cam_info, "mask_path", None):
        prior["alpha_mask"] = decode_mask(cam_info.mask_path)
    return Camera(colmap_id=cam_info.uid, R=cam_info.R, T=cam_info.T, FoVx=cam_info.FovX, FoVy=cam_info.FovY,
                  image=target, gt_alpha_mask=None, image_name=cam_info.image_name, uid=id,
                  data_device=args.data_device, device=device, **prior)


loadCam = load_cam


def cameraList_from_camInfos(cam_infos, resolution_scale, args, device="cuda"):
    return [load_cam(args, id, c, resolution_scale, device) for id, c in enumerate(cam_infos)]


def camera_to_JSON(id, camera) -> dict:
    """``utils/camera_utils.py:62-82`` for a ``CameraInfo``."""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = camera.R.transpose()
    Rt[:3, 3] = camera.T
    Rt[3, 3] = 1.0
    W2C = np.linalg.inv(Rt)
    pos = W2C[:3, 3]
    rot = W2C[:3, :3]
    return {"id": id, "img_name": camera.image_name, "width": camera.width, "height": camera.height,
            "position": pos.tolist(), "rotation": [x.tolist() for x in rot],
            "fy": fov2focal(camera.FovY, camera.height), "fx": fov2focal(camera.FovX, camera.width)}


def searchForMaxIteration(folder: str) -> int:
    return max(int(fname.split("_")[-1]) for fname in os.listdir(folder))


class Scene:
    """``scene/__init__.py:21-93``.  defer_cameras: stop after the host work (readers, ``input.ply``, ``cameras.json``,
    shuffle, ``cameras_extent``, the model's initialisation) and leave the images to a later ``load_cameras()``.
    depth_prior_mode: the ``OptimizationParams.depth_prior_mode`` the scene will be trained with; read only with
    ``args.depths``.  Priors without a ``depth_params.json`` are raw monocular maps, meaningless under the fixed identity
    affine of ``"l1"``: that combination is a ``ValueError``."""

    def __init__(self, args, gaussians, load_iteration=None, shuffle=True, resolution_scales=[1.0], *,
                 defer_cameras=False, device="cuda", depth_prior_mode="l1"):
        self.model_path = args.model_path
        self.loaded_iter = None
        self.gaussians = gaussians
        self.args = args
        self.device = device
        self.resolution_scales = list(resolution_scales)
        if load_iteration:
            if load_iteration == -1:
                self.loaded_iter = searchForMaxIteration(os.path.join(self.model_path, "point_cloud"))
            else:
                self.loaded_iter = load_iteration
            print("Loading trained model at iteration {}".format(self.loaded_iter))
        self.train_cameras = {}
        self.test_cameras = {}
        depths = {"depths": args.depths} if getattr(args, "depths", "") else {}     # no prior: the readers' old calls
        masks = {"masks": args.masks} if getattr(args, "masks", "") else {}         # no masks: likewise

        if os.path.exists(os.path.join(args.source_path, "sparse")):
            scene_info = sceneLoadTypeCallbacks["Colmap"](args.source_path, args.images, args.eval, **depths, **masks)
        elif os.path.exists(os.path.join(args.source_path, "transforms_train.json")):
            print("Found transforms_train.json file, assuming Blender data set!")
            scene_info = sceneLoadTypeCallbacks["Blender"](args.source_path, args.white_background, args.eval, **depths,
                                                           **masks)
        else:
            raise ValueError(f"Could not recognize scene type of {args.source_path!r}: neither sparse/ nor "
                             f"transforms_train.json is there")
        self.scene_info = scene_info
        if depths and depth_prior_mode == "l1" and all(c.depth_params is None for c in scene_info.train_cameras):
            raise ValueError(f"depths={args.depths!r} without sparse/0/depth_params.json: raw depth priors have no scale or "
                             f"offset, so depth_prior_mode='l1' (a fixed identity affine) is meaningless on them; train "
                             f"with depth_prior_mode='aligned_l1' or 'pearson', which fit the alignment per frame")

        if not self.loaded_iter:
            os.makedirs(self.model_path, exist_ok=True)
            with open(scene_info.ply_path, "rb") as src_file, \
                    open(os.path.join(self.model_path, "input.ply"), "wb") as dest_file:
                dest_file.write(src_file.read())
            camlist = list(scene_info.test_cameras or []) + list(scene_info.train_cameras or [])
            json_cams = [camera_to_JSON(id, cam) for id, cam in enumerate(camlist)]
            with open(os.path.join(self.model_path, "cameras.json"), "w") as file:
                json.dump(json_cams, file)

        if shuffle:
            random.shuffle(scene_info.train_cameras)  # Multi-res consistent random shuffling
            random.shuffle(scene_info.test_cameras)

        self.cameras_extent = scene_info.nerf_normalization["radius"]
        if not defer_cameras:
            self.load_cameras()

        if self.loaded_iter:
            self.gaussians.load_ply(os.path.join(self.model_path, "point_cloud", "iteration_" + str(self.loaded_iter),
                                                 "point_cloud.ply"))
            # upstream 3DGS: the exposures trained with the model, if it was trained with any
            exposure_file = os.path.join(self.model_path, "point_cloud", "iteration_" + str(self.loaded_iter),
                                         "exposure.json")
            if os.path.exists(exposure_file):
                self.gaussians.pretrained_exposures = load_exposures(exposure_file, device=self.gaussians._xyz.device)
        else:
            self.gaussians.create_from_pcd(scene_info.point_cloud, self.cameras_extent)

    def load_cameras(self):
        for resolution_scale in self.resolution_scales:
            self.train_cameras[resolution_scale] = cameraList_from_camInfos(self.scene_info.train_cameras,
                                                                            resolution_scale, self.args, self.device)
            self.test_cameras[resolution_scale] = cameraList_from_camInfos(self.scene_info.test_cameras,
                                                                           resolution_scale, self.args, self.device)

    def save(self, iteration):
        point_cloud_path = os.path.join(self.model_path, "point_cloud/iteration_{}".format(iteration))
        self.gaussians.save_ply(os.path.join(point_cloud_path, "point_cloud.ply"))
        if getattr(self.gaussians, "_exposure", None) is not None:
            save_exposures(os.path.join(point_cloud_path, "exposure.json"), self.gaussians.exposure_mapping,
                           self.gaussians._exposure)

    def getTrainCameras(self, scale=1.0):
        return self.train_cameras[scale]

    def getTestCameras(self, scale=1.0):
        return self.test_cameras[scale]


__all__ = ["ModelParams", "Camera", "MiniCam", "PoseCamera", "so3_exp", "pose_transforms", "Scene", "load_cam", "loadCam", "load_invdepth", "load_resolution",
           "mask_to_float",
           "cameraList_from_camInfos", "camera_to_JSON", "searchForMaxIteration"]
