"""GPU checks of model compression end to end (compress.compress_model / save_compressed / load_compressed / decode;
DESIGN.md §7.33) on a synthetic model of 2000 Gaussians at SH degree 3: what comes back from the file is codebook[index]
for the quantised groups and the float16 round trip for the others, rotations stay unit, the decoded model renders, and
the two lossless corners -- a codebook no smaller than the model, and all the weight on one row -- reproduce their input
bit for bit.  At SH degrees 0, 1 and 2, with every group quantised under dense weights, each stored codebook and index is
the restatement's Lloyd trajectory (``R.lloyd``) from the same init.  No image-quality number is pinned."""
import math

import numpy as np
import pytest
import torch

import kmeans_restate as R
from mvs_gaussian_splatting_amd import render
from mvs_gaussian_splatting_amd.compress import canonical_rotation, compress_model, load_compressed, save_compressed
from mvs_gaussian_splatting_amd.synthetic import PipelineParams, SceneConfig, make_scene

pytestmark = pytest.mark.gpu
P = 2000
ROWS = {"f_dc": "_features_dc", "f_rest": "_features_rest", "scaling": "_scaling", "rotation": "_rotation"}


@pytest.fixture(scope="module")
def scene(gpu_device):
    cfg = SceneConfig("vq", P, 3, 192, 112, 150.0, 150.0, math.log(0.05))
    model, cam, bg, _ = make_scene(cfg, seed=0)
    model.to(gpu_device)
    cam.to(gpu_device)
    return model, cam, bg.to(gpu_device)


def rows_of(model, name):
    t = getattr(model, ROWS[name]).detach()
    return canonical_rotation(t) if name == "rotation" else t.reshape(t.shape[0], -1)


def test_compress_save_load_decode_and_render(scene, gpu_device, tmp_path):
    model, cam, bg = scene
    cg = compress_model(model, codebook_size=256, iters=4, groups=("f_dc", "f_rest", "rotation"))
    path = str(tmp_path / "point_cloud_vq.npz")
    save_compressed(path, cg)
    back = load_compressed(path)
    assert back.nbytes() == cg.nbytes() < P * 62 * 4 / 4, "a quarter of the PLY payload at most"
    dec = back.decode(gpu_device)
    for name in ("f_dc", "f_rest", "rotation"):
        g = back.groups[name]
        assert g["index"].dtype == np.uint16 and g["codebook"].shape == (256, rows_of(model, name).shape[1])
        want = g["codebook"][g["index"].astype(np.int64)]
        got = dec[ROWS[name]].reshape(P, -1).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
        if name != "rotation":       # (its centres are renormalised after the last assign) every row sits at its rule's code
            assert np.array_equal(g["index"].astype(np.int32), R.assign(rows_of(model, name).cpu().numpy(), g["codebook"])[0])
    assert torch.equal(dec["_scaling"], model._scaling.half().float()) and set(back.groups["scaling"]) == {"half"}
    assert torch.equal(dec["_opacity"], model._opacity.half().float()) and torch.equal(dec["_xyz"], model._xyz)
    norm = np.linalg.norm(dec["_rotation"].double().cpu().numpy(), axis=1)
    assert np.abs(norm - 1).max() <= 8 * R.U, "decoded rotations are unit to float32 rounding"
    assert (dec["_rotation"][:, 0] >= 0).all()

    import copy
    twin = copy.copy(model)
    for attr in ROWS.values():
        setattr(twin, attr, dec[attr])
    twin._xyz, twin._opacity = dec["_xyz"], dec["_opacity"]
    img = render(cam, twin, PipelineParams(), bg)["render"]
    ref = render(cam, model, PipelineParams(), bg)["render"]
    assert img.shape == ref.shape and bool(torch.isfinite(img).all())
    mse = float(((img.detach() - ref.detach()) ** 2).mean())
    print(f"decoded against original: PSNR {10 * math.log10(1.0 / max(mse, 1e-20)):.2f} dB, payload {cg.nbytes()} bytes "
          f"against {P * 62 * 4}")


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_every_group_is_the_restatements_trajectory_from_the_same_init(gpu_device, degree):
    """All four groups quantised under dense weights at SH degree 0 (no f_rest), 1 (D = 9) and 2 (D = 24: the 16-step
    instantiation of the matrix-core kernel through the public entry), positions as float16."""
    n, K, iters, seed = 1500, 64, 3, 5
    arrays, w = R.model_arrays(n, degree)
    model = {k: torch.from_numpy(v).to(gpu_device) for k, v in arrays.items()}
    cg = compress_model(model, codebook_size=K, iters=iters, xyz_dtype="float16", seed=seed,
                        weights=torch.from_numpy(w).to(gpu_device))
    assert cg.sh_degree == degree and set(cg.groups) == set(ROWS) - ({"f_rest"} if degree == 0 else set())
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    perm = torch.randperm(n, generator=gen).numpy()
    for name, g in cg.groups.items():
        rows = arrays[ROWS[name]].reshape(n, -1)
        if name == "rotation":               # normalised on the device, as compress_model does, before it is clustered
            rows = canonical_rotation(model["_rotation"]).cpu().numpy()
        assert set(g) == {"codebook", "index"} and g["index"].dtype == np.uint16, name
        books, index, _, _ = R.lloyd(rows, R.first_distinct(rows, perm, K), iters, w)
        assert g["codebook"].shape == books[-1].shape == (K, {"f_dc": 3, "f_rest": 3 * ((degree + 1) ** 2 - 1), "scaling": 3,
                                                              "rotation": 4}[name]), name
        assert np.array_equal(g["index"].astype(np.int32), index), name
        if name != "rotation":
            assert np.array_equal(g["codebook"].view(np.uint32), books[-1].view(np.uint32)), name
        else:        # the last codebook of the trajectory, each centre back at unit length: a float32 norm of four terms
            q = g["codebook"].astype(np.float64)         # (at most 3 U relative) and one division (U), components <= 1
            assert np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 8 * R.U and (q[:, 0] >= 0).all()
            assert np.abs(q - R.canonical_rotation(books[-1])).max() <= 8 * R.U
    dec = cg.decode(gpu_device)
    assert cg.xyz.dtype == np.float16 and torch.equal(dec["_xyz"], model["_xyz"].half().float())
    g = cg.groups["scaling"]
    assert np.array_equal(dec["_scaling"].cpu().numpy().view(np.uint32), g["codebook"][g["index"].astype(np.int64)].view(np.uint32))
    assert dec["_features_rest"].shape == (n, (degree + 1) ** 2 - 1, 3)


def test_a_codebook_no_smaller_than_the_model_is_lossless(scene, gpu_device):
    model, _, _ = scene
    for size in (P, P + 1, 4096):
        dec = compress_model(model, codebook_size=size).decode(gpu_device)
        for name, attr in ROWS.items():
            assert torch.equal(dec[attr].reshape(P, -1), rows_of(model, name)), (size, name)


def test_all_the_weight_on_one_row_reproduces_that_row(scene, gpu_device):
    model, _, _ = scene
    row = 1234
    w = torch.zeros(P, device=gpu_device)
    w[row] = 2.5
    cg = compress_model(model, codebook_size=64, iters=3, weights=w)
    dec = cg.decode(gpu_device)
    for name, attr in ROWS.items():
        assert torch.equal(dec[attr].reshape(P, -1)[row], rows_of(model, name)[row]), name
