"""Generates tests/golden/scene_ingest.npz from the reference's own ingest layer (run ONLY where the reference checkout
exists; the fixture -- plain arrays -- is committed):

    python tests/golden/make_golden_scene.py

The generator writes a tiny scene into a temporary directory -- a COLMAP set (9 images, a PINHOLE and a SIMPLE_PINHOLE
camera, 40x30 and 64x48 PNGs of which one is RGBA, 50 points; binary and text files of the same content) and a Blender
set (5 + 4 RGBA frames) -- stores the bytes of those input files, and records what the reference computes from them:

  * scene/dataset_readers.py: readColmapSceneInfo for eval on / off (R, T, FovX, FovY, uid, names in sorted order, the
    split, nerf_normalization), the structured array storePly hands to ``plyfile`` and the arrays fetchPly builds from
    it (recording stub, the technique of make_golden_ply.py); readNerfSyntheticInfo for both backgrounds (poses, fovs,
    the composited bytes) and eval on / off;
  * utils/camera_utils.py: camera_to_JSON in the order scene/__init__.py lists the cameras (test, then train), and
    loadCam's resolution for -r in {-1, 1, 2, 4, 8, 20}, two resolution scales, and an image wider than 1600 pixels,
    with the PILtoTorch tensor it hands on (and the decoded pixels of those inputs);
  * scene/cameras.py: Camera.__init__'s original_image (with the alpha mask for the RGBA image) and its matrices.

Three things about the run, none of which touches the reference's text:
  - ``plyfile`` and ``simple_knn`` are absent: stub modules (make_golden_model.load_reference_model_module);
  - the Blender reader hands an int8 array to ``Image.fromarray(..., "RGB")``, which current Pillow rejects; the call is
    wrapped so that an int8 array is viewed as uint8 -- the bytes the Pillow versions that accepted it used;
  - ``.cuda()`` is neutralised and the cameras are built with data_device="cpu".
The reference's text reader of cameras.txt asserts PINHOLE, so it cannot read this scene's text files; the text files are
stored as inputs only (the host test checks that this package reads the same SceneInfo from them as from the binary ones).
"""
import json
import os
import struct
import sys
import tempfile
import types
from unittest import mock

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_model as gm  # noqa: E402
from make_golden_ply import RECORDED, RecordingPlyData, RecordingPlyElement  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


class PlyDataByName(RecordingPlyData):
    """fetchPly looks the element up by name (``plydata['vertex']``)."""

    @staticmethod
    def read(path):
        data, name = RECORDED["describe"]
        return PlyDataByName([RecordingPlyElement(data, name)])

    def __getitem__(self, key):
        return next(e for e in self.elements if e.name == key)


N_COLMAP, N_POINTS = 9, 50


def smooth_image(rng, w, h, channels):
    """A smooth pattern plus noise, so that resizing has something to interpolate."""
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 120 * np.sin(0.23 * x + 0.11 * y + k) for k in range(channels)], axis=2)
    img = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
    if channels == 4:
        img[:, :, 3] = np.clip(255 * (1.2 - np.hypot(x - w / 2, y - h / 2) / (0.5 * w)), 0, 255).astype(np.uint8)
    return img


def write_colmap(root, rng):
    os.makedirs(os.path.join(root, "images"))
    sparse = os.path.join(root, "sparse", "0")
    os.makedirs(sparse)
    cams = [(1, 1, "PINHOLE", 40, 30, [42.0, 43.5, 20.0, 15.0]), (2, 0, "SIMPLE_PINHOLE", 64, 48, [70.25, 32.0, 24.0])]
    order = [4, 0, 7, 2, 8, 1, 5, 3, 6]                            # file order differs from the sorted order
    images = []
    for image_id, k in enumerate(order, start=1):
        ang = 0.25 * (k - 4)                                        # an arc of cameras looking at (0, 0, 4)
        c2w = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        tilt = 0.05 * (k - 4)
        c2w = c2w @ np.array([[1, 0, 0], [0, np.cos(tilt), -np.sin(tilt)], [0, np.sin(tilt), np.cos(tilt)]])
        pos = np.array([0.0, 0.0, 4.0]) + c2w @ np.array([0.0, 0.0, -4.0 - 0.1 * k])
        Rw2c = c2w.T
        tvec = -Rw2c @ pos
        tr = np.trace(Rw2c)
        w = np.sqrt(max(1 + tr, 1e-12)) / 2
        q = np.array([w, (Rw2c[2, 1] - Rw2c[1, 2]) / (4 * w), (Rw2c[0, 2] - Rw2c[2, 0]) / (4 * w),
                      (Rw2c[1, 0] - Rw2c[0, 1]) / (4 * w)])
        cam = cams[k % 2]
        name = f"view_{k:02d}.png"
        channels = 4 if k == 3 else 3
        Image.fromarray(smooth_image(rng, cam[3], cam[4], channels)).save(os.path.join(root, "images", name))
        images.append((image_id, q, tvec, cam[0], name))
    pts = [(i + 1, rng.normal(0, 1.0, 3) + np.array([0, 0, 4.0]), rng.integers(0, 256, 3), float(rng.random()))
           for i in range(N_POINTS)]
    with open(os.path.join(sparse, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(cams)))
        for cid, mid, _, w_, h_, params in cams:
            f.write(struct.pack("<iiQQ", cid, mid, w_, h_) + struct.pack("<%dd" % len(params), *params))
    with open(os.path.join(sparse, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for cid, _, model, w_, h_, params in cams:
            f.write(f"{cid} {model} {w_} {h_} " + " ".join(repr(float(p)) for p in params) + "\n")
    with open(os.path.join(sparse, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(images)))
        for iid, q, t, cid, name in images:
            f.write(struct.pack("<i7di", iid, *q, *t, cid) + name.encode() + b"\x00")
            n2d = iid % 3                                          # a few 2D points, to be skipped by a reader
            f.write(struct.pack("<Q", n2d))
            for j in range(n2d):
                f.write(struct.pack("<ddq", 1.5 * j, 2.5 * j, -1))
    with open(os.path.join(sparse, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n")
        for iid, q, t, cid, name in images:
            f.write(f"{iid} " + " ".join(repr(float(v)) for v in list(q) + list(t)) + f" {cid} {name}\n")
            f.write(" ".join(f"{1.5 * j} {2.5 * j} -1" for j in range(iid % 3)) + "\n")
    with open(os.path.join(sparse, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(pts)))
        for pid, xyz, rgb, err in pts:
            f.write(struct.pack("<QdddBBBd", pid, *xyz, *[int(c) for c in rgb], err))
            f.write(struct.pack("<Q", 2) + struct.pack("<iiii", 1, 0, 2, 1))
    with open(os.path.join(sparse, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n")
        for pid, xyz, rgb, err in pts:
            f.write(f"{pid} " + " ".join(repr(float(v)) for v in xyz) + " " + " ".join(str(int(c)) for c in rgb) +
                    f" {err!r} 1 0 2 1\n")


def write_blender(root, rng):
    for split, n in (("train", 5), ("test", 4)):
        os.makedirs(os.path.join(root, split))
        frames = []
        for i in range(n):
            ang = 0.7 * i + (0.3 if split == "test" else 0.0)
            c2w = np.eye(4)
            c2w[:3, :3] = np.array([[np.cos(ang), -np.sin(ang) * 0.6, np.sin(ang) * 0.8],
                                    [np.sin(ang), np.cos(ang) * 0.6, -np.cos(ang) * 0.8], [0.0, 0.8, 0.6]])
            c2w[:3, 3] = c2w[:3, :3] @ np.array([0.0, 0.0, 4.0])
            frames.append({"file_path": f"./{split}/r_{i}", "rotation": 0.01, "transform_matrix": c2w.tolist()})
            Image.fromarray(smooth_image(rng, 40, 30, 4)).save(os.path.join(root, split, f"r_{i}.png"))
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, f, indent=1)


def store_files(out, root, prefix):
    for d, _, files in os.walk(root):
        for name in sorted(files):
            rel = os.path.relpath(os.path.join(d, name), root).replace(os.sep, "/")
            with open(os.path.join(d, name), "rb") as f:
                out[f"{prefix}/file/{rel}"] = np.frombuffer(f.read(), dtype=np.uint8).copy()


def record_cams(out, tag, cams):
    out[f"{tag}/names"] = np.array([c.image_name for c in cams])
    if not cams:
        return
    out[f"{tag}/R"] = np.stack([np.asarray(c.R) for c in cams])
    out[f"{tag}/T"] = np.stack([np.asarray(c.T) for c in cams])
    out[f"{tag}/fov_yx"] = np.array([[c.FovY, c.FovX] for c in cams], dtype=np.float64)
    out[f"{tag}/uid_w_h"] = np.array([[c.uid, c.width, c.height] for c in cams], dtype=np.int64)


def main():
    gm.load_reference_model_module()                               # sys.path and the stubs for plyfile / simple_knn
    import scene.dataset_readers as dr                            # noqa: E402  (the reference's modules)
    import scene.cameras as rc
    import utils.camera_utils as cu
    dr.PlyData, dr.PlyElement = PlyDataByName, RecordingPlyElement
    real_fromarray = Image.fromarray

    def fromarray(obj, mode=None):
        return real_fromarray(obj.view(np.uint8) if obj.dtype == np.int8 else obj)

    rng = np.random.default_rng(20240607)
    out = {}
    patches = [mock.patch.object(Image, "fromarray", fromarray),
               mock.patch.object(torch.Tensor, "cuda", lambda self, *a, **k: self)]
    with tempfile.TemporaryDirectory() as tmp, patches[0], patches[1]:
        colmap, blender = os.path.join(tmp, "colmap"), os.path.join(tmp, "blender")
        write_colmap(colmap, rng)
        write_blender(blender, rng)
        store_files(out, colmap, "colmap")
        store_files(out, blender, "blender")

        # ---- COLMAP ----
        for ev in (False, True):
            ply = os.path.join(colmap, "sparse/0/points3D.ply")
            assert not os.path.exists(ply)                         # the stub records; nothing is written
            info = dr.readColmapSceneInfo(colmap, "images", ev)
            tag = f"colmap/eval{int(ev)}"
            record_cams(out, f"{tag}/train", info.train_cameras)
            record_cams(out, f"{tag}/test", info.test_cameras)
            out[f"{tag}/translate"] = info.nerf_normalization["translate"]
            out[f"{tag}/radius"] = np.array(info.nerf_normalization["radius"])
            camlist = list(info.test_cameras) + list(info.train_cameras)
            out[f"{tag}/cameras_json"] = np.array(json.dumps([cu.camera_to_JSON(i, c) for i, c in enumerate(camlist)]))
        arr, name = RECORDED["describe"]
        assert name == "vertex"
        out["colmap/ply/field_names"] = np.array(list(arr.dtype.names))
        out["colmap/ply/field_formats"] = np.array([arr.dtype[n].str for n in arr.dtype.names])
        out["colmap/ply/raw_bytes"] = np.frombuffer(arr.tobytes(), dtype=np.uint8).copy()
        out["colmap/ply/itemsize_count"] = np.array([arr.dtype.itemsize, arr.shape[0]])
        for k in ("points", "colors", "normals"):
            out[f"colmap/pcd/{k}"] = np.asarray(getattr(info.point_cloud, k))

        # ---- loadCam / PILtoTorch / Camera ----
        info = dr.readColmapSceneInfo(colmap, "images", False)
        seen = {}

        class RecordingCamera:
            def __init__(self, **kw):
                seen.update(kw)

        real_camera = cu.Camera
        cu.Camera = RecordingCamera
        res_rows = []
        for cam_index in (0, 3):                                   # sorted order: view_00 (40x30 RGB), view_03 (64x48 RGBA)
            ci = info.train_cameras[cam_index]
            out[f"colmap/decoded/c{cam_index}"] = np.array(ci.image)      # the decoded input, for tests without Pillow
            for r in (-1, 1, 2, 4, 8, 20):
                for rs in (1.0, 2.0):
                    cu.loadCam(types.SimpleNamespace(resolution=r, data_device="cpu"), 5, ci, rs)
                    full = seen["image"] if seen["gt_alpha_mask"] is None else None
                    res_rows.append([cam_index, r, rs, seen["image"].shape[2], seen["image"].shape[1]])
                    if rs == 1.0 and r in (-1, 2, 20):
                        pil = ci.image.resize((seen["image"].shape[2], seen["image"].shape[1]))
                        t = torch.from_numpy(np.array(pil)) / 255.0
                        if r != -1:
                            out[f"loadcam/c{cam_index}_r{r}/piltotorch"] = t.permute(2, 0, 1).contiguous().numpy()
                        assert full is None or torch.equal(full, t.permute(2, 0, 1)[:3])
                        gt, mask = t.permute(2, 0, 1)[:3], (t.permute(2, 0, 1)[3:4] if t.shape[2] == 4 else None)
                        cam = real_camera(colmap_id=ci.uid, R=ci.R, T=ci.T, FoVx=ci.FovX, FoVy=ci.FovY, image=gt,
                                          gt_alpha_mask=mask, image_name=ci.image_name, uid=5, data_device="cpu")
                        out[f"loadcam/c{cam_index}_r{r}/original_image"] = cam.original_image.contiguous().numpy()
                        if r == -1:
                            for k in ("world_view_transform", "projection_matrix", "full_proj_transform", "camera_center"):
                                out[f"camera/c{cam_index}/{k}"] = getattr(cam, k).contiguous().numpy()
        wide = types.SimpleNamespace(image=Image.fromarray(rng.integers(0, 256, (20, 1700, 3), dtype=np.uint8)), uid=1,
                                     R=np.eye(3), T=np.zeros(3), FovX=1.0, FovY=1.0, image_name="wide")
        for r in (-1, 1, 2):
            cu.loadCam(types.SimpleNamespace(resolution=r, data_device="cpu"), 0, wide, 1.0)
            res_rows.append([-1, r, 1.0, seen["image"].shape[2], seen["image"].shape[1]])
        cu.Camera = real_camera
        out["loadcam/resolutions"] = np.array(res_rows, dtype=np.float64)     # cam (-1: 1700x20), -r, scale, width, height

        # ---- Blender ----
        for white in (False, True):
            for ev in (False, True):
                info = dr.readNerfSyntheticInfo(blender, white, ev)
                tag = f"blender/white{int(white)}/eval{int(ev)}"
                record_cams(out, f"{tag}/train", info.train_cameras)
                record_cams(out, f"{tag}/test", info.test_cameras)
                out[f"{tag}/translate"] = info.nerf_normalization["translate"]
                out[f"{tag}/radius"] = np.array(info.nerf_normalization["radius"])
                if not ev and not white:
                    out["blender/rgba"] = np.stack([np.array(Image.open(c.image_path).convert("RGBA"))
                                                    for c in info.train_cameras])
                if not ev:
                    out[f"blender/white{int(white)}/composite"] = np.stack([np.array(c.image) for c in info.train_cameras])
            ci = info.train_cameras[1]
            cu.Camera = RecordingCamera
            cu.loadCam(types.SimpleNamespace(resolution=2, data_device="cpu"), 1, ci, 1.0)
            cu.Camera = real_camera
            cam = real_camera(colmap_id=ci.uid, R=ci.R, T=ci.T, FoVx=ci.FovX, FoVy=ci.FovY, image=seen["image"],
                              gt_alpha_mask=seen["gt_alpha_mask"], image_name=ci.image_name, uid=1, data_device="cpu")
            out[f"blender/white{int(white)}/r2_original_image"] = cam.original_image.contiguous().numpy()
        assert RECORDED["describe"][0].shape[0] == 100_000         # the random cloud went to the stub, not into the fixture

    path = os.path.join(OUT, "scene_ingest.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
