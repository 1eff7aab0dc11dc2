"""Training masks without a GPU: the float64 restatement of the masked losses against the unmasked loss,
against finite differences and at Z = 0; the entry points' exports, ABI and refusals; the readers, ``decode_mask``,
``Camera(alpha_mask=)`` and ``load_cam`` on scenes written under ``tmp_path``."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import ingest_restate
import masked_loss_restate as R
from mvs_gaussian_splatting_amd import _lib, dataset_readers as dr, masked_loss as ml, scene as sc
from mvs_gaussian_splatting_amd.trainer import OptimizationParams

GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_ingest.npz")
ENTRY_POINTS = ("gsr_masked_l1_dssim_workspace_bytes", "gsr_masked_l1_dssim_loss_fwd_bwd", "gsr_alpha_mask_workspace_bytes",
                "gsr_alpha_mask_loss_fwd_bwd")
BAD, CAPACITY, ALIGN = -1, -2, -3


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("lam", R.LAMBDAS)
def test_all_ones_mask_is_the_unmasked_loss(shape, lam):
    x, gt = (t.double() for t in R.images(shape))
    ones = torch.ones(shape[1:], dtype=torch.float64)
    want = float(R.l1_dssim(x, gt, lam))
    for normalize in R.NORMALIZE:
        got = float(R.masked_l1_dssim(x, gt, ones, lam, normalize))
        assert abs(got - want) <= 1e-12, (normalize, got, want)


@pytest.mark.parametrize("normalize", R.NORMALIZE)
@pytest.mark.parametrize("kind", ["ones", "edge15", "soft"])
def test_restated_gradient_against_finite_differences(normalize, kind):
    shape = (3, 9, 11)
    x, gt = (t.double() for t in R.images(shape))
    m = (R.mask("edge5", 9, 11) if kind == "edge15" else R.mask(kind, 9, 11)).double()
    x.requires_grad_(True)
    for lam in R.LAMBDAS:
        assert torch.autograd.gradcheck(lambda t: R.masked_l1_dssim(t, gt, m, lam, normalize), (x,), eps=1e-6, atol=1e-7,
                                        rtol=1e-5)
    a = (0.01 + 0.98 * torch.rand(9, 11, dtype=torch.float64, generator=torch.Generator().manual_seed(4))).requires_grad_(True)
    for mode in ml.ALPHA_MODES:
        assert torch.autograd.gradcheck(lambda t: R.alpha_mask(t, m, mode), (a,), eps=1e-7, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("lam", R.LAMBDAS)
def test_an_empty_mask_gives_zero_and_zero_gradients(lam):
    shape = (3, 9, 11)
    x, gt = R.images(shape)
    zeros = torch.zeros(9, 11)
    for normalize in R.NORMALIZE:
        value, grad = R.value_and_grad(R.masked_l1_dssim, x, gt, zeros, lam, normalize, dtype=torch.float64)
        assert value == 0.0 and not grad.any(), normalize
    # the gradient is m times something: zero wherever the mask is, whatever the mode
    m = R.mask("edge5", 9, 11)
    for normalize in R.NORMALIZE:
        _, grad = R.value_and_grad(R.masked_l1_dssim, x, gt, m, lam, normalize, dtype=torch.float64)
        assert not grad[:, :, 5:].any() and (lam == 1.0 or grad[:, :, :5].abs().min() > 0)


def test_clamped_alpha_has_no_gradient_in_the_restatement():
    a = torch.tensor([[0.0, 1.0, 0.5, R.ALPHA_LO, R.ALPHA_HI, 1e-7]], dtype=torch.float64)
    m = torch.tensor([[1.0, 0.0, 1.0, 0.0, 1.0, 0.0]], dtype=torch.float64)
    value, grad = R.value_and_grad(R.alpha_mask, a, m, "bce", dtype=torch.float64)
    assert grad[0, 0] == 0 and grad[0, 1] == 0 and grad[0, 5] == 0 and grad[0, 2] != 0 and grad[0, 3] != 0 and grad[0, 4] != 0
    assert np.isfinite(value) and value > 0


# ---- ABI and refusals ------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points_and_the_abi_versions_agree():
    import mvs_gaussian_splatting_amd as pkg
    assert pkg.masked_l1_dssim_loss is ml.masked_l1_dssim_loss and pkg.alpha_mask_loss is ml.alpha_mask_loss
    assert {"masked_l1_dssim_loss", "alpha_mask_loss"} <= set(pkg.__all__)
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and re.search(r"\b(int|size_t) " + name + r"\(", header), name
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 45
    const = lambda n: int(re.search(rf"#define GSR_{n} (\d+)", header).group(1))      # noqa: E731
    assert {"image": const("MASKED_LOSS_NORM_IMAGE"), "mask": const("MASKED_LOSS_NORM_MASK")} == ml.NORMALIZE
    assert {"l1": const("ALPHA_MASK_L1"), "bce": const("ALPHA_MASK_BCE")} == ml.ALPHA_MODES
    assert const("MASKED_LOSS_RECORD_WORDS") == ml.RECORD_WORDS
    assert (_lib.MASKED_LOSS_NORM_IMAGE, _lib.MASKED_LOSS_NORM_MASK, _lib.ALPHA_MASK_L1, _lib.ALPHA_MASK_BCE) == (0, 1, 0, 1)


def test_workspaces_hold_the_maps_and_one_partial_per_workgroup():
    lib = _lib.load()
    for c, h, w in ((1, 1, 1), (3, 5, 7), (3, 16, 16), (3, 17, 33), (3, 1080, 1920)):
        b = lib.gsr_masked_l1_dssim_workspace_bytes(c, h, w)
        tiles = c * -(-h // 16) * -(-w // 16)
        assert b % 256 == 0 and b >= 4 * (3 * c * h * w + 2 * tiles) + 8 * 1024
        assert b <= 4 * (3 * c * h * w + 2 * tiles) + 8 * 1024 + 512
    assert lib.gsr_masked_l1_dssim_workspace_bytes(0, 4, 4) == 0 and lib.gsr_masked_l1_dssim_workspace_bytes(3, -1, 4) == 0
    for h, w in ((1, 1), (16, 16), (1080, 1920)):
        b = lib.gsr_alpha_mask_workspace_bytes(h, w)
        assert b % 256 == 0 and 8 * min(1024, -(-h * w // 256)) <= b <= 8 * 1024


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    buf = (C.c_char * (1 << 16))()
    p = (C.addressof(buf) + 255) // 256 * 256
    Cn, H, W = 3, 4, 5
    wb = lib.gsr_masked_l1_dssim_workspace_bytes(Cn, H, W)
    good = [p, p, p, Cn, H, W, 0.2, 0, p, p, p, wb]
    fn = lib.gsr_masked_l1_dssim_loss_fwd_bwd
    for n, value, code in ((0, None, BAD), (1, None, BAD), (2, None, BAD), (8, None, BAD), (10, None, BAD), (3, 0, BAD),
                           (3, 65536, BAD), (4, 0, BAD), (5, -1, BAD), (6, float("nan"), BAD), (6, 1.5, BAD), (6, -0.1, BAD),
                           (7, 2, BAD), (7, -1, BAD), (11, wb - 1, CAPACITY), (0, p + 2, ALIGN), (2, p + 1, ALIGN),
                           (9, p + 2, ALIGN), (8, p + 4, ALIGN), (10, p + 128, ALIGN)):
        args = list(good)
        args[n] = value
        assert fn(*args, None) == code, (n, value)
    assert fn(*good[:7], 7, *good[8:], None) == BAD and b"normalize" in lib.gsr_last_error()
    assert fn(p, p, p, Cn, H, W, 0.2, 1, p, None, p, wb - 1, None) == CAPACITY           # a NULL gradient is legal
    wa = lib.gsr_alpha_mask_workspace_bytes(H, W)
    good = [p, p, H, W, 1, p, p, p, wa]
    fn = lib.gsr_alpha_mask_loss_fwd_bwd
    for n, value, code in ((0, None, BAD), (1, None, BAD), (5, None, BAD), (7, None, BAD), (2, 0, BAD), (3, -2, BAD),
                           (4, 2, BAD), (4, -1, BAD), (8, wa - 1, CAPACITY), (0, p + 1, ALIGN), (6, p + 2, ALIGN),
                           (5, p + 4, ALIGN), (7, p + 4, ALIGN)):
        args = list(good)
        args[n] = value
        assert fn(*args, None) == code, (n, value)
    assert fn(p, p, H, W, 0, p, None, p, wa - 1, None) == CAPACITY


def test_python_wrappers_refuse_bad_arguments_and_cpu_tensors():
    x, gt, m = torch.zeros(3, 4, 5), torch.zeros(3, 4, 5), torch.ones(4, 5)
    for args, kw, err in (((x.numpy(), gt, m), {}, TypeError), ((x, gt, "m"), {}, TypeError), ((x.double(), gt, m), {}, TypeError),
                          ((x, gt, m.bool()), {}, TypeError), ((x, gt.half(), m), {}, TypeError),
                          ((x[0], gt[0], m), {}, ValueError), ((x, torch.zeros(3, 4, 6), m), {}, ValueError),
                          ((x, gt, torch.ones(5, 4)), {}, ValueError), ((x, gt, torch.ones(3, 4, 5)), {}, ValueError),
                          ((x, gt, torch.ones(1, 1, 4, 5)), {}, ValueError), ((x, gt, m.to("meta")), {}, ValueError),
                          ((x, gt, m), {"normalize": "pixels"}, ValueError), ((x, gt, m), {"normalize": 1}, ValueError),
                          ((x, gt, m), {"lambda_dssim": 1.5}, ValueError), ((x, gt, m), {"lambda_dssim": "0.2"}, ValueError),
                          ((torch.zeros(3, 0, 5), torch.zeros(3, 0, 5), torch.ones(0, 5)), {}, ValueError)):
        with pytest.raises(err):
            ml.masked_l1_dssim_loss(*args, **kw)
    for normalize in R.NORMALIZE:
        for mask in (m, m[None]):
            with pytest.raises(_lib.GsrError, match="no CPU path"):
                ml.masked_l1_dssim_loss(x, gt, mask, normalize=normalize)
    a = torch.zeros(1, 4, 5)
    for args, kw, err in (((a.numpy(), m), {}, TypeError), ((a.double(), m), {}, TypeError), ((a, m.long()), {}, TypeError),
                          ((torch.zeros(2, 4, 5), m), {}, ValueError), ((torch.zeros(5), torch.zeros(5)), {}, ValueError),
                          ((a, torch.ones(4, 6)), {}, ValueError), ((a, m), {"mode": "huber"}, ValueError),
                          ((a, m), {"mode": 1}, ValueError)):
        with pytest.raises(err):
            ml.alpha_mask_loss(*args, **kw)
    for mode in ml.ALPHA_MODES:
        with pytest.raises(_lib.GsrError, match="no CPU path"):
            ml.alpha_mask_loss(a, m[None], mode=mode)
        with pytest.raises(_lib.GsrError, match="no CPU path"):
            ml.alpha_mask_loss(a[0], m, mode=mode)


def test_optimization_and_model_params_defaults():
    opt = OptimizationParams()
    assert (opt.mask_photometric, opt.mask_normalize, opt.lambda_alpha_mask, opt.alpha_mask_mode) == (True, "image", 0.0, "bce")
    assert OptimizationParams(mask_normalize="mask", lambda_alpha_mask=0.1, alpha_mask_mode="l1", mask_photometric=False)
    assert sc.ModelParams().masks == "" and sc.ModelParams(masks="masks").masks == "masks"


# ---- ingest ----------------------------------------------------------------------------------------------------------------
try:
    from PIL import Image as pil
except ImportError:
    pil = None
needs_pillow = pytest.mark.skipif(pil is None, reason="the readers open images with Pillow")


def write_scene(prefix, root, keep=lambda rel: True):
    gold = np.load(GOLDEN)
    for key in gold.files:
        head = f"{prefix}/file/"
        if key.startswith(head) and keep(key[len(head):]):
            path = os.path.join(root, key[len(head):])
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "wb") as f:
                f.write(gold[key].tobytes())
    return str(root)


def write_mask(path, array):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    pil.fromarray(np.asarray(array, dtype=np.uint8)).save(path)


def mask_array(name, h=6, w=8):
    rng = np.random.default_rng(sum(name.encode()))
    return (rng.integers(0, 2, size=(h, w)) * 255).astype(np.uint8)


@needs_pillow
def test_colmap_scene_finds_masks_under_both_names_and_refuses_a_missing_one(tmp_path):
    root = write_scene("colmap", tmp_path / "src", lambda rel: not rel.endswith(".bin"))
    plain = dr.readColmapSceneInfo(root, "images", True)
    cams = plain.train_cameras + plain.test_cameras
    assert all(c.mask_path is None for c in cams)
    assert all(c.mask_path is None for c in dr.readColmapSceneInfo(root, "images", True, masks="").train_cameras)
    train = sorted(plain.train_cameras, key=lambda c: c.image_name)
    # half the training images by stem, half by COLMAP's <file name>.png; the first one under both: the stem wins
    by_stem = {c.image_name for c in train[::2]}
    for c in train:
        stem = os.path.join(root, "masks", c.image_name + ".png")
        full = os.path.join(root, "masks", os.path.basename(c.image_path) + ".png")
        assert stem != full
        write_mask(stem if c.image_name in by_stem else full, mask_array(c.image_name))
    write_mask(os.path.join(root, "masks", os.path.basename(train[0].image_path) + ".png"), mask_array("other"))
    for masks in ("masks", os.path.join(root, "masks")):                         # relative to the scene, or absolute
        info = dr.readColmapSceneInfo(root, "images", True, masks=masks)
        assert [c.image_name for c in info.train_cameras] == [c.image_name for c in plain.train_cameras]
        for c in info.train_cameras:
            name = c.image_name if c.image_name in by_stem else os.path.basename(c.image_path)
            assert c.mask_path == os.path.join(root, "masks", name + ".png")
            assert np.array_equal(dr.decode_mask(c.mask_path), mask_array(c.image_name))
        assert info.test_cameras and all(c.mask_path is None for c in info.test_cameras)
    # the held-out images need none; with every image in the training set one is missing, and it is named
    held_out = plain.test_cameras[0].image_name
    with pytest.raises(FileNotFoundError, match=held_out):
        dr.readColmapSceneInfo(root, "images", False, masks="masks")
    # through Scene: ModelParams.masks reaches the reader, "" leaves its call as it was
    args = sc.ModelParams(source_path=root, model_path=str(tmp_path / "out"), eval=True, masks="masks")
    scene = sc.Scene(args, FakeGaussians(), shuffle=False, defer_cameras=True)
    assert all(c.mask_path for c in scene.scene_info.train_cameras)
    args = sc.ModelParams(source_path=root, model_path=str(tmp_path / "out2"), eval=True)
    scene = sc.Scene(args, FakeGaussians(), shuffle=False, defer_cameras=True)
    assert all(c.mask_path is None for c in scene.scene_info.train_cameras)


class FakeGaussians:
    def create_from_pcd(self, pcd, extent):
        pass


@needs_pillow
def test_blender_scene_with_masks(tmp_path):
    root = write_scene("blender", tmp_path / "src")
    plain = dr.readNerfSyntheticInfo(root, True, True)
    assert all(c.mask_path is None for c in plain.train_cameras + plain.test_cameras)
    for c in plain.train_cameras:
        write_mask(os.path.join(root, "sil", c.image_name + ".png"), mask_array(c.image_name))
    info = dr.readNerfSyntheticInfo(root, True, True, masks="sil")
    assert info.train_cameras and all(c.mask_path == os.path.join(root, "sil", c.image_name + ".png") for c in info.train_cameras)
    assert all(c.mask_path is None for c in info.test_cameras)
    missing = info.train_cameras[0].image_name
    os.remove(os.path.join(root, "sil", missing + ".png"))
    with pytest.raises(FileNotFoundError, match=missing):
        dr.readNerfSyntheticInfo(root, True, True, masks="sil")


def test_camera_info_keeps_its_positional_arguments_and_gains_mask_path():
    c = dr.CameraInfo(1, np.eye(3), np.zeros(3), 0.5, 0.6, None, "a/b.png", "b", 8, 6, np.zeros(3))
    assert c.mask_path is None and c.depth_path == "" and c._replace(mask_path="m.png").mask_path == "m.png"
    assert "mask_path" in dr.CameraInfo._fields


@needs_pillow
def test_decode_mask_any_channel_non_zero_keeps_the_pixel(tmp_path):
    grey = np.array([[0, 1, 128, 255], [0, 0, 7, 0]], np.uint8)
    want = np.array([[0, 255, 255, 255], [0, 0, 255, 0]], np.uint8)
    write_mask(str(tmp_path / "grey.png"), grey)
    assert np.array_equal(dr.decode_mask(str(tmp_path / "grey.png")), want)
    rgb = np.zeros((2, 4, 3), np.uint8)
    rgb[0, 1, 2], rgb[0, 2, 0], rgb[0, 3], rgb[1, 2, 1] = 1, 128, (255, 255, 255), 7          # one channel each, then all
    write_mask(str(tmp_path / "rgb.png"), rgb)
    got = dr.decode_mask(str(tmp_path / "rgb.png"))
    assert got.dtype == np.uint8 and got.shape == (2, 4) and np.array_equal(got, want)
    rgba = np.concatenate([np.zeros((2, 4, 3), np.uint8), grey[:, :, None]], axis=2)          # only the alpha channel is set
    write_mask(str(tmp_path / "rgba.png"), rgba)
    assert np.array_equal(dr.decode_mask(str(tmp_path / "rgba.png")), want)
    pil.fromarray(grey > 0).save(str(tmp_path / "bits.png"))                                     # a 1-bit file
    assert np.array_equal(dr.decode_mask(str(tmp_path / "bits.png")), want)


def _camera(H, W, gt_alpha_mask=None, **kw):
    return sc.Camera(1, np.eye(3), np.zeros(3), 0.6, 0.5, torch.full((3, H, W), 0.5), gt_alpha_mask, "v", 0,
                     data_device="cpu", device="cpu", **kw)


def test_camera_keeps_the_mask_beside_the_image():
    cam = _camera(6, 8)
    assert cam.alpha_mask is None and sc.PoseCamera(cam).alpha_mask is None
    m = mask_array("cam")
    m[0, :3] = (0, 255, 51)
    cam = _camera(6, 8, alpha_mask=m)
    assert cam.alpha_mask.shape == (1, 6, 8) and cam.alpha_mask.dtype == torch.float32
    assert torch.equal(cam.alpha_mask[0], torch.from_numpy(m).float() / 255.0) and float(cam.alpha_mask[0, 0, 2]) == np.float32(51) / np.float32(255)
    assert torch.equal(cam.original_image, torch.full((3, 6, 8), 0.5)), "the mask is not multiplied into the target"
    assert sc.PoseCamera(cam).alpha_mask is cam.alpha_mask
    # gt_alpha_mask keeps its meaning: it multiplies the target and leaves no alpha_mask
    cam = _camera(6, 8, gt_alpha_mask=torch.from_numpy(m).float()[None] / 255.0)
    assert cam.alpha_mask is None and torch.equal(cam.original_image[0], 0.5 * torch.from_numpy(m).float() / 255.0)
    # a float mask at the camera's size is clamped; another size or dtype is refused
    f = torch.linspace(-0.5, 1.5, 48).reshape(6, 8)
    assert torch.equal(_camera(6, 8, alpha_mask=f).alpha_mask[0], f.clamp(0.0, 1.0))
    assert torch.equal(_camera(6, 8, alpha_mask=f[None]).alpha_mask[0], f.clamp(0.0, 1.0))
    with pytest.raises(ValueError):
        _camera(6, 8, alpha_mask=torch.zeros(3, 4))
    with pytest.raises(TypeError):
        _camera(6, 8, alpha_mask=torch.zeros(6, 8, dtype=torch.int32))


@needs_pillow
@pytest.mark.parametrize("size", [(8, 6), (9, 5), (16, 12)], ids=str)
def test_a_mask_of_another_size_is_resized_as_the_photographs_are(size):
    """(W, H) of the mask file against a 16 x 12 camera: half size, an odd size, the camera's own."""
    w, h = size
    m = mask_array("resize", h, w)
    cam = _camera(12, 16, alpha_mask=m)
    resized = m if (w, h) == (16, 12) else ingest_restate.resize(m[:, :, None], (16, 12))[:, :, 0]
    want = (torch.from_numpy(np.ascontiguousarray(resized)).float() / 255.0).clamp(0.0, 1.0)
    assert cam.alpha_mask.shape == (1, 12, 16) and torch.equal(cam.alpha_mask[0], want)
    assert float(cam.alpha_mask.min()) >= 0.0 and float(cam.alpha_mask.max()) <= 1.0
    if (w, h) != (16, 12):
        assert ((cam.alpha_mask > 0) & (cam.alpha_mask < 1)).any(), "a resized hard mask has soft edges"


@needs_pillow
def test_load_cam_forwards_the_mask_to_the_camera(tmp_path, monkeypatch):
    path = str(tmp_path / "cam.png")
    m = mask_array("load", 6, 8)
    write_mask(path, np.stack([m, 0 * m, 0 * m], axis=2))                                # a multi-channel file
    seen = []

    class Spy(sc.Camera):
        def __init__(self, **kw):
            seen.append(set(kw))
            super().__init__(**kw)
    monkeypatch.setattr(sc, "Camera", Spy)
    monkeypatch.setattr(sc.image_ingest, "load_image", lambda array, size, device, composite_bg=None: torch.zeros(3, size[1], size[0]))
    monkeypatch.setattr(sc, "decode_image", lambda info: None)
    image = pil.fromarray(np.zeros((12, 16, 3), np.uint8))
    args = sc.ModelParams(resolution=2, data_device="cpu")
    base = dr.CameraInfo(3, np.eye(3), np.zeros(3), 0.5, 0.6, image, "cam.png", "cam", 16, 12)
    cam = sc.load_cam(args, 0, base, 1.0, device="cpu")
    assert cam.alpha_mask is None and "alpha_mask" not in seen[0]
    cam = sc.load_cam(args, 0, base._replace(mask_path=path), 1.0, device="cpu")
    assert "alpha_mask" in seen[1] and torch.equal(cam.alpha_mask[0], torch.from_numpy(m).float() / 255.0)
