"""CPU-side checks of the depth-prior layer (csrc/depth_prior.hip, csrc/depth_prior_math.h; depth_prior.py; the readers'
and ``scene.Camera``'s prior fields; trainer.depth_prior_weight): the restatement the GPU tests compare
against (tests/depth_prior_restate.py) against central differences and against the kernel's own body built by the host
compiler (tests/depth_prior_host_check.cpp), depth-map ingest on temporary COLMAP-text and Blender scenes, ``Camera``'s
host arithmetic on CPU tensors, the ABI and every refusal -- all before a GPU is asked for."""
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import depth_prior_restate as R
from mvs_gaussian_splatting_amd import _lib, dataset_readers as dr, depth_prior as dp, scene as sc
from mvs_gaussian_splatting_amd.trainer import OptimizationParams, depth_prior_weight

GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_ingest.npz")
ENTRY_POINTS = ("gsr_depth_prior_workspace_bytes", "gsr_depth_prior_fwd_bwd")
BAD, CAPACITY, ALIGN = -1, -2, -3


# ---- the restatement against central differences ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
def test_restated_gradients_against_central_differences(mode):
    x, y, w = R.case(13, 17, seed=1)
    res = R.evaluate(x, y, w, mode, scale=0.4, offset=0.1)
    assert res.valid.sum() > 100 and (~res.valid).sum() > 20
    x64 = x.astype(np.float64)
    frozen = (res.fit.s, res.fit.t) if mode == "aligned_l1" else None
    assert abs(R.loss64(x64, y, w, mode, 0.4, 0.1, frozen) - res.loss) <= 1e-13 * max(1.0, abs(res.loss))
    h, worst = 1e-6, 0.0
    for i in range(x.size):
        e = np.zeros(x.size)
        e[i] = h
        e = e.reshape(x.shape)
        fd = (R.loss64(x64 + e, y, w, mode, 0.4, 0.1, frozen) - R.loss64(x64 - e, y, w, mode, 0.4, 0.1, frozen)) / (2 * h)
        if mode != "pearson" and res.valid.reshape(-1)[i]:
            assert abs(res.residual.reshape(-1)[i]) > h, "a kink inside the difference stencil: the case checks nothing"
        worst = max(worst, abs(fd - res.grad64.reshape(-1)[i]))
    print(f"[depth prior] {mode}: closed form against central differences, max error {worst:.3e}")
    assert worst <= 1e-8
    assert not res.grad64[~res.valid].any()


def test_the_cases_are_well_conditioned_and_no_sign_is_a_decision():
    """What the GPU bars rest on: both variances keep > 5 % of their mean squares, and under the restatement's own fit no
    valid residual of aligned_l1 is within the first-order bound of 0 (so the GPU test excludes nothing on these inputs)."""
    for H, W in ((13, 17), (64, 65), (520, 520)):
        x, y, w = R.case(H, W)
        res = R.evaluate(x, y, w, "aligned_l1")
        n = int(res.valid.sum())
        assert res.cond > 0.05 and not res.fit.degenerate
        assert abs(res.fit.s - 0.4) < 0.05 and abs(res.fit.t - 0.1) < 0.05 and R.evaluate(x, y, w, "pearson").fit.r > 0.9
        bound = 64 * (n + 8) * R.U / res.cond * res.a                              # a = w / Sw: the GPU test's own bound
        assert int((res.valid & (np.abs(res.residual) <= bound)).sum()) == 0


def test_degenerate_rule_of_the_restatement():
    x, y, w = R.case(13, 17)
    for xx, yy, ww in ((x[:1, :1], y[:1, :1], np.ones((1, 1), np.float32)), (np.full_like(x, 0.7), y, w),
                       (x, y, np.zeros_like(w)), (x, np.full_like(y, np.nan), w)):
        for mode in ("aligned_l1", "pearson"):
            res = R.evaluate(xx, yy, ww, mode)
            assert res.loss == 0.0 and not res.grad.any() and res.record[3:7].tolist() == [1.0, 0.0, 0.0, 1.0]


# ---- the header built by the host compiler -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """``csrc/depth_prior_math.h`` built by the host compiler from ``tests/depth_prior_host_check.cpp`` into a program of its
    own, with the kernel's ``-ffp-contract=off``."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or \
        os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    folder = tmp_path_factory.mktemp("depth_prior_host")
    exe = str(folder / "depth_prior_host_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc"),
                    os.path.join(ROOT, "tests", "depth_prior_host_check.cpp"), "-o", exe], check=True)

    def run(n, sums, scale, offset, pixels, x, y, w):
        path = str(folder / "pixels.bin")
        rec = np.zeros(x.size, dtype=[("x", "<f4"), ("y", "<f4"), ("w", "<f4")])
        rec["x"], rec["y"], rec["w"] = x.reshape(-1), y.reshape(-1), w.reshape(-1)
        with open(path, "wb") as f:
            f.write(struct.pack("<q", n) + np.asarray(sums, dtype="<f8").tobytes() +
                    struct.pack("<dddq", scale, offset, pixels, x.size) + rec.tobytes())
        lines = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines()
        head = lines[0].split()
        assert head[0] == "fit"
        fit = np.array([int(v, 16) for v in head[1:]], dtype=np.uint64).view(np.float64)
        rows = [line.split() for line in lines[1:]]
        valid = np.array([int(r[0]) for r in rows], dtype=bool)
        terms = np.array([[int(v, 16) for v in r[1:7]] for r in rows], dtype=np.uint64).reshape(-1, 6)
        grads = np.array([[int(v, 16) for v in r[7:10]] for r in rows], dtype=np.uint32).reshape(-1, 3)
        return fit, valid, terms, grads
    return run


@pytest.mark.parametrize("shape", [(13, 17), (64, 65)])
def test_host_build_of_the_header_gives_the_restatements_bits(host_check, shape):
    x, y, w = R.case(*shape)
    x[0, 0], w[0, 0] = np.nan, 0.0                                  # a non-finite render at a masked pixel
    x[1, 1], w[1, 1] = np.inf, 1.0                                  # ... and at a weighted one: invalid too
    w[2, 2] = -1.0
    res = {m: R.evaluate(x, y, w, m, scale=0.4, offset=0.1) for m in R.MODES}
    n = int(res["l1"].valid.sum())
    fit, valid, terms, grads = host_check(n, res["l1"].sums, 0.4, 0.1, float(x.size), x, y, w)
    assert np.array_equal(valid, res["l1"].valid.reshape(-1)) and not valid[0] and not valid[shape[1] + 1]
    assert np.array_equal(fit.view(np.uint64), np.array(res["pearson"].fit, dtype=np.float64).view(np.uint64)), \
        "the fit from the given sums differs in its float64 bits"
    assert np.array_equal(terms[valid].T, res["l1"].terms.view(np.uint64)) and not terms[~valid].any()
    for k, mode in enumerate(R.MODES):
        assert np.array_equal(grads[:, k], res[mode].grad.reshape(-1).view(np.uint32)), f"{mode}: a gradient differs in its bits"
        assert res[mode].grad.any()


def test_host_build_marks_degenerate_sums(host_check):
    x, y, w = R.case(13, 17)
    for xx, ww in ((np.full_like(x, 0.7), w), (x, np.zeros_like(w))):
        res = R.evaluate(xx, y, ww, "pearson")
        fit, _, _, grads = host_check(int(res.valid.sum()), res.sums, 1.0, 0.0, float(x.size), xx, y, ww)
        want = np.array(res.fit, dtype=np.float64)
        assert fit[11] == 1.0 and fit[7:11].tolist() == [0.0, 1.0, 0.0, 0.0] and not grads[:, 1:].any()
        assert np.array_equal(np.isnan(fit), np.isnan(want)) and np.array_equal(fit[~np.isnan(fit)], want[~np.isnan(want)])


# ---- ABI and refusals ----------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points_and_the_abi_versions_agree():
    import mvs_gaussian_splatting_amd as pkg
    assert pkg.depth_prior_loss is dp.depth_prior_loss and "depth_prior_loss" in pkg.__all__
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and re.search(r"\b(int|size_t) " + name + r"\(", header), name
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("gsr_depth_prior_")) == sorted(ENTRY_POINTS)
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 44
    const = lambda n: int(re.search(rf"#define GSR_DEPTH_PRIOR_{n} (\d+)", header).group(1))      # noqa: E731
    assert (const("BLOCK"), const("MAX_BLOCKS"), const("SUM_WORDS"), const("RECORD_WORDS"), const("FIT_COUNT_WORD")) == \
        (dp.BLOCK, dp.MAX_BLOCKS, dp.SUM_WORDS, dp.RECORD_WORDS, dp.FIT_COUNT_WORD)
    assert {m: const(m.upper()) for m in R.MODES} == dp.MODES


def test_workspace_holds_the_fit_block_and_one_partial_per_workgroup():
    lib = _lib.load()
    last = 0
    for h, w in ((1, 1), (1, 256), (1, 257), (256, 1024), (520, 520), (1080, 1920), (1 << 14, 1 << 14)):
        b = lib.gsr_depth_prior_workspace_bytes(h, w)
        blocks = min(dp.MAX_BLOCKS, -(-h * w // dp.BLOCK))
        assert b % 256 == 0 and b >= 8 * (dp.FIT_COUNT_WORD + dp.SUM_WORDS + 10 * blocks) and last <= b <= 8 * (32 + 10 * 1024) + 256
        last = b


def test_entry_point_refuses_bad_arguments_before_any_hip_call():
    lib = _lib.load()
    buf = (C.c_char * (1 << 17))()
    p = (C.addressof(buf) + 255) // 256 * 256
    H, W = 4, 5
    wb = lib.gsr_depth_prior_workspace_bytes(H, W)
    good = [p, p, p, H, W, 0, 1.0, 0.0, p, p, p, wb]
    fn = lib.gsr_depth_prior_fwd_bwd
    for n, value, code in ((0, None, BAD), (1, None, BAD), (8, None, BAD), (10, None, BAD), (3, 0, BAD), (4, -1, BAD),
                           (3, 1 << 15, BAD), (5, 3, BAD), (5, -1, BAD), (6, float("nan"), BAD), (7, float("inf"), BAD),
                           (11, wb - 1, CAPACITY), (0, p + 2, ALIGN), (2, p + 1, ALIGN), (9, p + 2, ALIGN), (8, p + 4, ALIGN),
                           (10, p + 128, ALIGN)):
        args = list(good)
        args[n] = value
        if n == 3 and value == 1 << 15:
            args[4] = 1 << 14                                      # 2^29 pixels
        assert fn(*args, None) == code, (n, value)
    assert fn(*good[:6], float("nan"), 0.0, *good[8:], None) == BAD and b"finite" in lib.gsr_last_error()
    # a NULL weight and a NULL gradient are legal: the next refusal in line is reached with both
    assert fn(p, p, None, H, W, 0, 1.0, 0.0, p, None, p, wb - 1, None) == CAPACITY


def test_depth_prior_loss_refuses_bad_arguments_and_cpu_tensors():
    x = torch.zeros(1, 4, 5)
    y, w = torch.zeros(1, 4, 5), torch.ones(4, 5)
    for args, kw, err in (((x.numpy(), y), {}, TypeError), ((x, "y"), {}, TypeError), ((x, y, 1.0), {}, TypeError),
                          ((x.double(), y), {}, TypeError), ((x, y.half()), {}, TypeError), ((x, y, w.long()), {}, TypeError),
                          ((torch.zeros(2, 4, 5), torch.zeros(2, 4, 5)), {}, ValueError), ((torch.zeros(5), torch.zeros(5)), {}, ValueError),
                          ((torch.zeros(1, 0, 5), torch.zeros(1, 0, 5)), {}, ValueError),
                          ((x, torch.zeros(1, 4, 6)), {}, ValueError), ((x, y, torch.ones(5, 4)), {}, ValueError),
                          ((x, y, torch.ones(3, 4, 5)), {}, ValueError),
                          ((x, y.to("meta")), {}, ValueError), ((x, y, w.to("meta")), {}, ValueError),
                          ((x, y), {"mode": "huber"}, ValueError), ((x, y), {"mode": 0}, ValueError),
                          ((x, y), {"scale": float("nan")}, ValueError), ((x, y), {"offset": float("inf")}, ValueError),
                          ((x, y), {"scale": "1"}, ValueError), ((x, y), {"offset": None}, ValueError)):
        with pytest.raises(err):
            dp.depth_prior_loss(*args, **kw)
    big = torch.zeros(1, dtype=torch.float32).expand(1, 1 << 15, 1 << 14)                 # 2^29 pixels, one element
    with pytest.raises(ValueError, match="2\\^28"):
        dp.depth_prior_loss(big, big)
    for mode in R.MODES:
        with pytest.raises(_lib.GsrError, match="no CPU path"):
            dp.depth_prior_loss(x, y, w, mode=mode)
        with pytest.raises(_lib.GsrError, match="no CPU path"):
            dp.depth_prior_loss(x[0], y[0], mode=mode, return_record=True)


# ---- the schedule --------------------------------------------------------------------------------------------------------
def test_optimization_params_defaults_and_the_weight_schedule():
    opt = OptimizationParams()
    assert (opt.depth_l1_weight_init, opt.depth_l1_weight_final, opt.depth_prior_mode) == (1.0, 0.01, "l1")
    # exp(log(v)) is v to within two roundings
    assert depth_prior_weight(opt, 0) == pytest.approx(1.0, rel=4e-16, abs=0.0)
    assert depth_prior_weight(opt, opt.iterations) == pytest.approx(0.01, rel=4e-16, abs=0.0)
    assert depth_prior_weight(opt, opt.iterations // 2) == pytest.approx(0.1, rel=1e-12)
    small = OptimizationParams(iterations=50, depth_l1_weight_init=0.5, depth_l1_weight_final=0.125)
    assert depth_prior_weight(small, 0) == pytest.approx(0.5, rel=4e-16) and depth_prior_weight(small, 50) == pytest.approx(0.125, rel=4e-16)
    assert depth_prior_weight(small, 25) == pytest.approx(0.25, rel=1e-12) and depth_prior_weight(small, 80) == depth_prior_weight(small, 50)
    assert depth_prior_weight(OptimizationParams(depth_l1_weight_init=0.0, depth_l1_weight_final=0.0), 10) == 0.0
    assert sc.ModelParams().depths == "" and sc.ModelParams(depths="depths").depths == "depths"


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


def write_prior(path, array_u16):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    pil.fromarray(np.asarray(array_u16, dtype=np.uint16)).save(path)


def prior_array(name, h=6, w=8):
    rng = np.random.default_rng(sum(name.encode()))
    return rng.integers(0, 65536, size=(h, w), dtype=np.uint16)


@needs_pillow
def test_colmap_text_scene_with_depth_priors(tmp_path):
    root = write_scene("colmap", tmp_path, lambda rel: not rel.endswith(".bin"))
    plain = dr.readColmapSceneInfo(root, "images", True)
    names = sorted(c.image_name for c in plain.train_cameras + plain.test_cameras)
    assert all(c.depth_path == "" and c.depth_params is None for c in plain.train_cameras + plain.test_cameras)
    for name in names:
        write_prior(os.path.join(root, "depths", name + ".png"), prior_array(name))
    # without depth_params.json: paths, no parameters
    info = dr.readColmapSceneInfo(root, "images", True, depths="depths")
    assert [c.image_name for c in info.train_cameras] == [c.image_name for c in plain.train_cameras]
    for c in info.train_cameras:
        assert c.depth_path == os.path.join(root, "depths", c.image_name + ".png") and c.depth_params is None
    assert len(info.test_cameras) == 2 and all(c.depth_path == "" and c.depth_params is None for c in info.test_cameras)
    # with it: every entry gets the median of the POSITIVE scales
    scales = {name: s for name, s in zip(names, (2.0, -1.0, 0.5, 4.0, 1.0, 0.0, 3.0, 8.0, 0.25))}
    with open(os.path.join(root, "sparse/0/depth_params.json"), "w") as f:
        json.dump({name: {"scale": s, "offset": 0.125 * i} for i, (name, s) in enumerate(scales.items())}, f)
    med = float(np.median([s for s in scales.values() if s > 0]))
    assert med == 2.0
    info = dr.readColmapSceneInfo(root, "images", False, depths="depths")
    assert len(info.train_cameras) == 9 and not info.test_cameras
    for c in info.train_cameras:
        i = names.index(c.image_name)
        assert c.depth_params == {"scale": scales[c.image_name], "offset": 0.125 * i, "med_scale": med}
    # a missing PNG of a training camera is refused by name; the one of a held-out test camera is not needed
    held_out = dr.readColmapSceneInfo(root, "images", True).test_cameras[0].image_name
    os.remove(os.path.join(root, "depths", held_out + ".png"))
    assert len(dr.readColmapSceneInfo(root, "images", True, depths="depths").train_cameras) == 7
    with pytest.raises(FileNotFoundError, match=held_out + ".png"):
        dr.readColmapSceneInfo(root, "images", False, depths="depths")


class FakeGaussians:
    def create_from_pcd(self, pcd, extent):
        pass


@needs_pillow
def test_blender_scene_with_depth_priors_and_the_scene_rule(tmp_path):
    root = write_scene("blender", tmp_path / "src")
    plain = dr.readNerfSyntheticInfo(root, True, True)
    for c in plain.train_cameras + plain.test_cameras:
        write_prior(os.path.join(root, "mono", c.image_name + ".png"), prior_array(c.image_name))
    info = dr.readNerfSyntheticInfo(root, True, True, depths="mono")
    assert info.train_cameras and info.test_cameras
    for c in info.train_cameras:
        assert c.depth_path == os.path.join(root, "mono", c.image_name + ".png") and c.depth_params is None
    assert all(c.depth_path == "" for c in info.test_cameras)
    both = dr.readNerfSyntheticInfo(root, True, False, depths="mono")
    assert len(both.train_cameras) == len(plain.train_cameras) + len(plain.test_cameras) and all(c.depth_path for c in both.train_cameras)
    # raw priors under the identity affine are refused; the fitted modes take them
    args = sc.ModelParams(source_path=root, model_path=str(tmp_path / "out"), white_background=True, depths="mono")
    with pytest.raises(ValueError, match="aligned_l1.*pearson"):
        sc.Scene(args, FakeGaussians(), shuffle=False, defer_cameras=True)
    scene = sc.Scene(args, FakeGaussians(), shuffle=False, defer_cameras=True, depth_prior_mode="pearson")
    assert all(c.depth_path for c in scene.scene_info.train_cameras)
    first = info.train_cameras[0].image_name
    os.remove(os.path.join(root, "mono", first + ".png"))
    with pytest.raises(FileNotFoundError, match=first + ".png"):
        dr.readNerfSyntheticInfo(root, True, True, depths="mono")


def test_camera_info_with_the_old_positional_arguments_still_constructs():
    c = dr.CameraInfo(1, np.eye(3), np.zeros(3), 0.5, 0.6, None, "a/b.png", "b", 8, 6)
    assert c.composite_bg is None and c.depth_path == "" and c.depth_params is None
    c = dr.CameraInfo(1, np.eye(3), np.zeros(3), 0.5, 0.6, None, "a/b.png", "b", 8, 6, np.zeros(3))
    assert c.depth_path == "" and c._replace(depth_path="d.png").depth_path == "d.png"
    assert dr.CameraInfo._fields[-2:] == ("depth_path", "depth_params")


@needs_pillow
def test_decode_refuses_what_is_not_a_16_bit_single_channel_png(tmp_path):
    a = prior_array("a")
    good = str(tmp_path / "good.png")
    write_prior(good, a)
    got = dr.decode_invdepth(good)
    assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32) / np.float32(65536.0))
    assert np.array_equal(got.astype(np.float64) * 65536.0, a.astype(np.float64)), "uint16 / 65536 is exact in float32"
    eight = str(tmp_path / "eight.png")
    pil.fromarray((a >> 8).astype(np.uint8)).save(eight)
    rgb = str(tmp_path / "rgb.png")
    pil.fromarray(np.zeros((6, 8, 3), np.uint8)).save(rgb)
    for path in (eight, rgb):
        with pytest.raises(ValueError, match=os.path.basename(path)):
            dr.decode_invdepth(path)
        with pytest.raises(ValueError, match=os.path.basename(path)):
            sc.load_invdepth(path, (8, 6), "cpu")


def _camera(H, W, **kw):
    return sc.Camera(1, np.eye(3), np.zeros(3), 0.6, 0.5, torch.zeros(3, H, W), None, "v", 0, data_device="cpu", device="cpu", **kw)


def test_camera_without_a_prior_has_none():
    cam = _camera(6, 8)
    assert cam.invdepthmap is None and cam.depth_mask is None and cam.depth_reliable is False
    pose = sc.PoseCamera(cam)
    assert pose.invdepthmap is None and pose.depth_reliable is False


@needs_pillow
def test_load_invdepth_and_the_cameras_host_arithmetic(tmp_path):
    a = prior_array("prior", 12, 16)
    a[0, :4] = (0, 1, 65535, 32768)
    path = str(tmp_path / "prior.png")
    write_prior(path, a)
    raw = torch.from_numpy(a.astype(np.float32)) / 65536.0
    same = sc.load_invdepth(path, (16, 12), "cpu")
    assert same.shape == (1, 12, 16) and same.dtype == torch.float32 and torch.equal(same[0], raw)
    assert same[0, 0, :4].tolist() == [0.0, 2.0 ** -16, 65535 / 65536, 0.5]
    for size in ((8, 6), (7, 5), (20, 9)):                                              # (W, H): down, odd, mixed
        got = sc.load_invdepth(path, size, "cpu")
        want = torch.nn.functional.interpolate(raw[None, None], size=(size[1], size[0]), mode="bilinear",
                                               align_corners=False, antialias=False)[0]
        assert got.shape == (1, size[1], size[0]) and torch.equal(got, want)
    m = sc.load_invdepth(path, (8, 6), "cpu")
    # no parameters: the map as it is, reliable, a mask of ones
    cam = _camera(6, 8, invdepthmap=m)
    assert torch.equal(cam.invdepthmap, m) and torch.equal(cam.depth_mask, torch.ones(1, 6, 8)) and cam.depth_reliable is True
    assert cam.invdepthmap.dtype == cam.depth_mask.dtype == torch.float32
    assert sc.PoseCamera(cam).invdepthmap is cam.invdepthmap and sc.PoseCamera(cam).depth_reliable is True
    # negatives are clamped before the affine; [H, W] input is accepted
    neg = m[0].clone()
    neg[0, 0] = -0.25
    cam = _camera(6, 8, invdepthmap=neg, depth_params={"scale": 2.0, "offset": 0.5, "med_scale": 2.0})
    want = neg.clamp(min=0.0)[None] * 2.0 + 0.5
    assert torch.equal(cam.invdepthmap, want) and float(cam.invdepthmap[0, 0, 0]) == 0.5 and cam.depth_reliable
    # the unreliable rule: exactly 0.2 med and 5 med are reliable, just outside is not
    med = 1.5
    for scale, reliable in ((0.2 * med, True), (5 * med, True), (np.nextafter(0.2 * med, 0.0), False),
                            (np.nextafter(5 * med, 100.0), False), (med, True)):
        cam = _camera(6, 8, invdepthmap=m, depth_params={"scale": float(scale), "offset": 0.25, "med_scale": med})
        assert cam.depth_reliable is reliable, scale
        assert torch.equal(cam.depth_mask, torch.full((1, 6, 8), 1.0 if reliable else 0.0))
        assert torch.equal(cam.invdepthmap, m * float(scale) + 0.25)                 # the affine applies either way: scale > 0
    # a scale that is not positive: unreliable against a positive median, and no affine
    for scale in (0.0, -1.0):
        cam = _camera(6, 8, invdepthmap=m, depth_params={"scale": scale, "offset": 0.25, "med_scale": med})
        assert cam.depth_reliable is False and not cam.depth_mask.any() and torch.equal(cam.invdepthmap, m)
    with pytest.raises(RuntimeError):
        _camera(6, 8, invdepthmap=torch.zeros(1, 5, 8))


@needs_pillow
def test_load_cam_forwards_the_prior_to_the_camera(tmp_path, monkeypatch):
    """``load_cam`` with the GPU image chain replaced by zeros: a ``CameraInfo`` with a prior reaches ``Camera`` with the
    resized map and its parameters; one without builds the camera with the arguments it always had."""
    a = prior_array("cam", 12, 16)
    path = str(tmp_path / "cam.png")
    write_prior(path, a)
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
    assert cam.invdepthmap is None and "invdepthmap" not in seen[0] and "depth_params" not in seen[0]
    params = {"scale": 2.0, "offset": 0.5, "med_scale": 2.0}
    cam = sc.load_cam(args, 0, base._replace(depth_path=path, depth_params=params), 1.0, device="cpu")
    want = sc.load_invdepth(path, (8, 6), "cpu") * 2.0 + 0.5
    assert cam.invdepthmap.shape == (1, 6, 8) and torch.equal(cam.invdepthmap, want) and cam.depth_reliable
    assert {"invdepthmap", "depth_params"} <= seen[1]


@needs_pillow
def test_reader_does_not_import_cv2(tmp_path):
    import sys
    path = str(tmp_path / "prior.png")
    write_prior(path, prior_array("cv2"))
    code = ("import sys; sys.modules['cv2'] = None\n"
            "from mvs_gaussian_splatting_amd import scene\n"
            f"m = scene.load_invdepth({path!r}, (4, 3), 'cpu')\n"
            "assert m.shape == (1, 3, 4)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
