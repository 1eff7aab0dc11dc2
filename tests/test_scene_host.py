"""Host side of scene loading (``dataset_readers``, ``scene``, ``image_ingest``'s tables) against what the reference
computed on the fixture scene of ``tests/golden/scene_ingest.npz`` (``tests/golden/make_golden_scene.py``), and the
integer resize against Pillow byte for byte.  Nothing here touches a GPU."""
import importlib.util
import json
import os
import random
import re

import numpy as np
import pytest
import torch

from mvs_gaussian_splatting_amd import _lib, dataset_readers as dr, image_ingest, scene as sc

import ingest_restate

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_ingest.npz")
needs_pillow = pytest.mark.skipif(importlib.util.find_spec("PIL") is None, reason="the readers open images with Pillow")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def write_scene(gold, prefix, root, keep=lambda rel: True):
    for key in gold.files:
        head = f"{prefix}/file/"
        if key.startswith(head) and keep(key[len(head):]):
            path = os.path.join(root, key[len(head):])
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "wb") as f:
                f.write(gold[key].tobytes())
    return str(root)


def check_cams(gold, tag, cams):
    assert [c.image_name for c in cams] == list(gold[f"{tag}/names"])
    if not cams:
        return
    assert np.array_equal(np.stack([c.R for c in cams]), gold[f"{tag}/R"])                    # float64, same numpy ops
    assert np.array_equal(np.stack([c.T for c in cams]), gold[f"{tag}/T"])
    assert np.array_equal(np.array([[c.FovY, c.FovX] for c in cams]), gold[f"{tag}/fov_yx"])
    assert np.array_equal(np.array([[c.uid, c.width, c.height] for c in cams]), gold[f"{tag}/uid_w_h"])


def test_abi_declares_the_ingest_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gsr.h")).read()
    lib = _lib.load()
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 19
    for name in ("gsr_image_composite_u8", "gsr_image_resize_u8", "gsr_image_to_float_chw"):
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\(", header)
    # argument validation happens before anything is launched
    assert lib.gsr_image_composite_u8(None, 4, 4, 0.0, 0.0, 0.0, None, None) == -1
    assert lib.gsr_image_composite_u8(8, 4, 4, 0.0, 2.0, 0.0, 8, None) == -1 and b"background" in lib.gsr_last_error()
    assert lib.gsr_image_resize_u8(8, 2, 4, 4, 2, 2, None, None, 0, None, None, 0, None, 8, None) == -1
    assert lib.gsr_image_resize_u8(8, 3, 4, 4, 2, 2, None, None, 0, None, None, 0, None, 8, None) == -1
    assert lib.gsr_image_to_float_chw(8, 1, 4, 4, 8, None) == -1
    assert lib.gsr_image_to_float_chw(8, 3, 0, 4, 8, None) == -1


@needs_pillow
@pytest.mark.parametrize("ev", [False, True])
def test_colmap_reader_reproduces_the_reference(gold, tmp_path, ev):
    root = write_scene(gold, "colmap", tmp_path)
    info = dr.readColmapSceneInfo(root, "images", ev)
    tag = f"colmap/eval{int(ev)}"
    check_cams(gold, f"{tag}/train", info.train_cameras)
    check_cams(gold, f"{tag}/test", info.test_cameras)
    assert len(info.test_cameras) == (2 if ev else 0)                                           # indices 0 and 8 of 9
    assert np.array_equal(info.nerf_normalization["translate"], gold[f"{tag}/translate"])
    assert info.nerf_normalization["radius"] == float(gold[f"{tag}/radius"])
    camlist = list(info.test_cameras) + list(info.train_cameras)
    assert json.dumps([sc.camera_to_JSON(i, c) for i, c in enumerate(camlist)]) == str(gold[f"{tag}/cameras_json"])
    # points3D.bin became points3D.ply: the array the reference hands to plyfile, behind plyfile's header
    assert info.ply_path == os.path.join(root, "sparse/0/points3D.ply")
    raw = open(info.ply_path, "rb").read()
    names, formats = list(gold["colmap/ply/field_names"]), list(gold["colmap/ply/field_formats"])
    ply_type = {"<f4": "float", "|u1": "uchar"}
    header = "ply\nformat binary_little_endian 1.0\nelement vertex 50\n" + \
        "".join(f"property {ply_type[f]} {n}\n" for n, f in zip(names, formats)) + "end_header\n"
    assert raw == header.encode() + gold["colmap/ply/raw_bytes"].tobytes()
    assert list(gold["colmap/ply/itemsize_count"]) == [27, 50]
    for k in ("points", "colors", "normals"):
        got = getattr(info.point_cloud, k)
        assert got.dtype == gold[f"colmap/pcd/{k}"].dtype and np.array_equal(got, gold[f"colmap/pcd/{k}"])


@needs_pillow
def test_colmap_text_files_give_the_same_scene(gold, tmp_path):
    a = dr.readColmapSceneInfo(write_scene(gold, "colmap", tmp_path / "bin"), "images", True)
    b = dr.readColmapSceneInfo(write_scene(gold, "colmap", tmp_path / "txt", lambda rel: not rel.endswith(".bin")),
                               None, True)                                  # images=None falls back to "images"
    assert not os.path.exists(tmp_path / "txt" / "sparse/0/images.bin")
    for x, y in ((a.train_cameras, b.train_cameras), (a.test_cameras, b.test_cameras)):
        assert [c.image_name for c in x] == [c.image_name for c in y]
        for cx, cy in zip(x, y):
            assert np.array_equal(cx.R, cy.R) and np.array_equal(cx.T, cy.T)
            assert (cx.FovX, cx.FovY, cx.uid, cx.width, cx.height) == (cy.FovX, cy.FovY, cy.uid, cy.width, cy.height)
    assert a.nerf_normalization["radius"] == b.nerf_normalization["radius"]
    for k in ("points", "colors", "normals"):
        assert np.array_equal(getattr(a.point_cloud, k), getattr(b.point_cloud, k))
    assert open(a.ply_path, "rb").read() == open(b.ply_path, "rb").read()


def test_unsupported_camera_model_raises():
    with pytest.raises(ValueError, match="OPENCV"):
        dr.colmap_fov(dr.ColmapCamera(1, "OPENCV", 40, 30, np.ones(8)))
    fy, fx = dr.colmap_fov(dr.ColmapCamera(1, "SIMPLE_RADIAL", 40, 30, np.array([50.0, 20.0, 15.0, 0.01])))
    assert (fy, fx) == (dr.focal2fov(50.0, 30), dr.focal2fov(50.0, 40))


def test_qvec2rotmat_is_a_rotation():
    q = np.array([0.5, -0.5, 0.5, 0.5])
    R = dr.qvec2rotmat(q)
    assert np.allclose(R @ R.T, np.eye(3)) and np.isclose(np.linalg.det(R), 1.0)
    assert np.allclose(R, [[0, -1, 0], [0, 0, 1], [-1, 0, 0]])


@needs_pillow
@pytest.mark.parametrize("white", [False, True])
def test_blender_reader_reproduces_the_reference(gold, tmp_path, white):
    root = write_scene(gold, "blender", tmp_path)
    for ev in (False, True):
        info = dr.readNerfSyntheticInfo(root, white, ev)
        tag = f"blender/white{int(white)}/eval{int(ev)}"
        check_cams(gold, f"{tag}/train", info.train_cameras)
        check_cams(gold, f"{tag}/test", info.test_cameras)
        assert len(info.train_cameras) == (5 if ev else 9)
        assert np.array_equal(info.nerf_normalization["translate"], gold[f"{tag}/translate"])
        assert info.nerf_normalization["radius"] == float(gold[f"{tag}/radius"])
    # no points3d.ply in the set: 100 000 random points inside the synthetic bounds, written once
    assert info.point_cloud.points.shape == (100_000, 3) and np.abs(info.point_cloud.points).max() <= 1.3
    assert np.array_equal(info.point_cloud.normals, np.zeros((100_000, 3), np.float32))
    before = os.path.getmtime(info.ply_path)
    again = dr.readNerfSyntheticInfo(root, white, False)
    assert os.path.getmtime(info.ply_path) == before and np.array_equal(again.point_cloud.points, info.point_cloud.points)
    # the composite of :204-210, on the host chain: the bytes the reference's reader produced
    want = gold[f"blender/white{int(white)}/composite"]
    for i, cam in enumerate(again.train_cameras):
        assert cam.composite_bg.tolist() == ([1, 1, 1] if white else [0, 0, 0])
        rgba = dr.decode_image(cam)
        assert rgba.shape == (30, 40, 4)
        assert np.array_equal(image_ingest.composite_host(rgba, cam.composite_bg), want[i])


def test_load_resolution_matches_loadcam(gold):
    sizes = {0: (40, 30), 3: (64, 48), -1: (1700, 20)}
    rows = gold["loadcam/resolutions"]
    assert len(rows) == 27
    for cam, r, rs, w, h in rows:
        ow, oh = sizes[int(cam)]
        assert sc.load_resolution(ow, oh, int(r), float(rs)) == (int(w), int(h)), (cam, r, rs)
    assert sc.load_resolution(1700, 20, -1) == (1600, 18)


@needs_pillow
def test_host_chain_reproduces_piltotorch_and_the_masked_image(gold, tmp_path):
    root = write_scene(gold, "colmap", tmp_path)
    info = dr.readColmapSceneInfo(root, "images", False)
    for ci, r in ((0, -1), (0, 2), (0, 20), (3, -1), (3, 2), (3, 20)):
        cam = info.train_cameras[ci]
        a = dr.decode_image(cam)
        assert a.shape[2] == (4 if ci == 3 else 3)
        size = sc.load_resolution(cam.width, cam.height, r)
        got = image_ingest.load_image_host(a, size)
        assert torch.equal(got, torch.from_numpy(gold[f"loadcam/c{ci}_r{r}/original_image"]))
        if r != -1:
            full = torch.from_numpy(gold[f"loadcam/c{ci}_r{r}/piltotorch"])
            assert full.shape[0] == a.shape[2]
            mask = full[3:4] if ci == 3 else 1.0
            assert torch.equal(got, full[:3] * mask)
    bl = dr.readNerfSyntheticInfo(write_scene(gold, "blender", tmp_path / "b"), True, True)
    cam = bl.train_cameras[1]
    got = image_ingest.load_image_host(dr.decode_image(cam), (20, 15), composite_bg=cam.composite_bg)
    assert torch.equal(got, torch.from_numpy(gold["blender/white1/r2_original_image"]))
    with pytest.raises(ValueError, match="single-channel"):
        image_ingest.load_image_host(np.zeros((4, 4), np.uint8), (2, 2))


SIZE_PAIRS = [(97, 61, 12, 8), (640, 427, 160, 107), (333, 251, 167, 126), (2000, 1300, 1600, 1040),
              (2474, 1644, 1237, 822), (50, 40, 50, 20), (50, 40, 25, 40), (40, 30, 97, 61), (1700, 20, 1600, 18)]


@needs_pillow
@pytest.mark.parametrize("w,h,w2,h2", SIZE_PAIRS)
def test_integer_resize_equals_pillow(w, h, w2, h2):
    from PIL import Image
    rng = np.random.default_rng(w * 7 + h2)
    y, x = np.mgrid[0:h, 0:w]
    gradient = ((x[:, :, None] * np.array([1, 2, 3]) + y[:, :, None] * np.array([3, 1, 2])) % 256).astype(np.uint8)
    for img in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), gradient):
        want = np.array(Image.fromarray(img).resize((w2, h2)))
        got = ingest_restate.resize(img, (w2, h2))
        assert got.shape == want.shape and int((got != want).sum()) == 0
    grey = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if w * h < 100_000:
        assert np.array_equal(ingest_restate.resize(grey[:, :, None], (w2, h2))[:, :, 0],
                              np.array(Image.fromarray(grey).resize((w2, h2))))


def test_resize_tables_are_well_formed():
    for n_in, n_out in ((97, 12), (40, 97), (4946, 1600), (5, 1), (1, 7)):
        bounds, taps = image_ingest.resize_tables(n_in, n_out)
        assert bounds.dtype == taps.dtype == np.int32 and bounds.shape == (n_out, 2) and taps.shape[0] == n_out
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= n_in).all()
        assert (bounds[:, 1] <= taps.shape[1]).all()
        assert np.abs(taps.sum(1) - (1 << image_ingest.PRECISION_BITS)).max() <= taps.shape[1]     # weights sum to one
        assert np.abs(taps).sum(1).max() * 255 < 2 ** 31 - 2 ** 21                                # the int32 accumulator holds


class FakeGaussians:
    def __init__(self):
        self.calls = []

    def create_from_pcd(self, pcd, extent):
        self.calls.append(("create_from_pcd", pcd.points.shape, extent))

    def load_ply(self, path):
        self.calls.append(("load_ply", path))

    def save_ply(self, path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        open(path, "wb").write(b"ply")


@needs_pillow
def test_scene_host_side(gold, tmp_path):
    src = write_scene(gold, "colmap", tmp_path / "src")
    out = str(tmp_path / "out")
    args = sc.ModelParams(source_path=src, model_path=out, eval=True)
    assert args.resolution == -1 and args.images == "images" and args.sh_degree == 3
    with pytest.raises(TypeError):
        sc.ModelParams(no_such_field=1)
    g = FakeGaussians()
    random.seed(5)
    scene = sc.Scene(args, g, defer_cameras=True)
    assert open(os.path.join(out, "input.ply"), "rb").read() == open(os.path.join(src, "sparse/0/points3D.ply"), "rb").read()
    assert open(os.path.join(out, "cameras.json")).read() == str(gold["colmap/eval1/cameras_json"])
    assert scene.cameras_extent == float(gold["colmap/eval1/radius"])
    assert g.calls == [("create_from_pcd", (50, 3), scene.cameras_extent)]
    names = sorted(gold["colmap/eval1/train/names"])
    shuffled = [c.image_name for c in scene.scene_info.train_cameras]
    assert sorted(shuffled) == names and shuffled != names
    assert sorted(c.image_name for c in scene.scene_info.test_cameras) == sorted(gold["colmap/eval1/test/names"])
    random.seed(5)
    again = sc.Scene(args, FakeGaussians(), defer_cameras=True)
    assert [c.image_name for c in again.scene_info.train_cameras] == shuffled
    plain = sc.Scene(args, FakeGaussians(), shuffle=False, defer_cameras=True)
    assert [c.image_name for c in plain.scene_info.train_cameras] == names
    assert scene.train_cameras == {} and scene.loaded_iter is None
    # save, then load_iteration = -1 finds the highest iteration
    for it in (7, 30, 200):
        scene.save(it)
    os.remove(os.path.join(out, "cameras.json"))
    g2 = FakeGaussians()
    loaded = sc.Scene(args, g2, load_iteration=-1, shuffle=False, defer_cameras=True)
    assert loaded.loaded_iter == 200
    assert g2.calls == [("load_ply", os.path.join(out, "point_cloud", "iteration_200", "point_cloud.ply"))]
    assert not os.path.exists(os.path.join(out, "cameras.json"))          # a loaded scene writes nothing
    assert sc.Scene(args, FakeGaussians(), load_iteration=30, defer_cameras=True).loaded_iter == 30
    with pytest.raises(ValueError, match="scene type"):
        sc.Scene(sc.ModelParams(source_path=str(tmp_path / "nothing"), model_path=out), FakeGaussians(), defer_cameras=True)


@needs_pillow
def test_scene_detects_a_blender_set(gold, tmp_path):
    src = write_scene(gold, "blender", tmp_path / "src")
    g = FakeGaussians()
    scene = sc.Scene(sc.ModelParams(source_path=src, model_path=str(tmp_path / "out"), white_background=True), g,
                     shuffle=False, defer_cameras=True)
    assert scene.cameras_extent == float(gold["blender/white1/eval0/radius"])
    assert g.calls == [("create_from_pcd", (100_000, 3), scene.cameras_extent)]
    assert len(json.load(open(tmp_path / "out" / "cameras.json"))) == 9


@needs_pillow
def test_camera_matrices_match_the_reference(gold, tmp_path):
    info = dr.readColmapSceneInfo(write_scene(gold, "colmap", tmp_path), "images", False)
    for ci in (0, 3):
        c = info.train_cameras[ci]
        cam = sc.Camera(c.uid, c.R, c.T, c.FovX, c.FovY, torch.zeros(3, 4, 6), None, c.image_name, 5, data_device="cpu",
                        device="cpu")
        assert (cam.image_width, cam.image_height, cam.znear, cam.zfar, cam.uid, cam.colmap_id) == (6, 4, 0.01, 100.0, 5, c.uid)
        for k in ("world_view_transform", "projection_matrix", "full_proj_transform", "camera_center"):
            torch.testing.assert_close(getattr(cam, k), torch.from_numpy(gold[f"camera/c{ci}/{k}"]))
    mini = sc.MiniCam(6, 4, cam.FoVy, cam.FoVx, 0.01, 100.0, cam.world_view_transform, cam.full_proj_transform)
    torch.testing.assert_close(mini.camera_center, cam.camera_center)


def test_package_imports_without_pillow():
    import subprocess
    import sys
    code = ("import sys; sys.modules['PIL'] = None\n"
            "import mvs_gaussian_splatting_amd as m, mvs_gaussian_splatting_amd.scene, mvs_gaussian_splatting_amd.image_ingest\n"
            "assert m.Scene and m.load_image")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)
