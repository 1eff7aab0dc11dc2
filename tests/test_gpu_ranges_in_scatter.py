"""Tile ranges and tile order built by the rider workgroup of the tile sort's last scatter (run on the GPU box:
pytest -m gpu).

The two-level binning modes no longer launch ranges_and_order_from_sort_kernel behind the tile sort: one workgroup more
in the sort's last scatter launch runs the same body (binning.hip: radix_scatter_kernel with RIDER,
ranges_and_order_from_sort_body) at SORT_THREADS lanes.  The reference for the ranges is the same frame in the 64-bit key
mode, which reads them off the sorted keys (identify_tile_ranges): they must be equal exactly, and so must the image.
The tile order has no reference (inside a length bucket it follows LDS atomic arrival): it is checked as a permutation,
chunk by chunk of 8 * SORT_THREADS tiles, along which the length bucket never increases -- the order is built per chunk
(longest first inside each), which is what the compositing kernels are promised.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import small_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc")
SORT_THREADS = int(re.search(r"constexpr int SORT_THREADS = (\d+);", open(os.path.join(CSRC, "gsr_common.h")).read()).group(1))
RIDER_CHUNK = 8 * SORT_THREADS       # tiles the rider orders per pass
P = 30_000


def len_bucket(length):
    """binning.hip len_bucket on an int64 array."""
    length = np.asarray(length, dtype=np.int64)
    e = np.zeros_like(length)
    big = length >= 16
    e[big] = np.floor(np.log2(length[big])).astype(np.int64)
    e[big & ((np.int64(1) << e) > length)] -= 1
    b = 16 + (e - 4) * 8 + ((length >> np.maximum(e - 3, 0)) & 7)
    return np.where(big, np.minimum(b, 255), length)


def _align(x):
    return (x + 255) & ~255


def _tile_order_offset(lib, W, H):
    """gsr_common.h ImageLayout: final_T, n_contrib [W*H words], ranges [T,2], tile_max [T], tile_order [T]."""
    T = ((W + 15) // 16) * ((H + 15) // 16)
    o = _align(4 * W * H)
    o = _align(o + 4 * W * H)
    o = _align(o + 8 * T)
    o = _align(o + 4 * T)
    assert _align(o + 4 * T) == lib.gsr_image_bytes(W, H), "ImageLayout restated wrongly"
    return o, T


class _Frames:
    """One model and one set of workspaces; every frame goes into them."""

    def __init__(self, dev, W, H, cap=None):
        from mvs_gaussian_splatting_amd import _lib
        self.lib, self.dev, self.W, self.H, self.cap = _lib.load(), dev, W, H, cap
        self.model, self.cam, _, _ = small_scene(P=P, sh_degree=1, width=W, height=H, focal=0.6 * W, scale=0.03)
        self.model.to(dev)
        self.cam.to(dev)
        self.bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
        self.order_off, self.T = _tile_order_offset(self.lib, W, H)
        self.geom = torch.empty(self.lib.gsr_geom_bytes(P), dtype=torch.uint8, device=dev)
        self.img = torch.empty(self.lib.gsr_image_bytes(W, H), dtype=torch.uint8, device=dev)
        self.binning = None
        if cap is not None:
            self.nb = self.lib.gsr_binning_bytes(cap, P, W, H, _lib.BINNING_TWO_LEVEL)
            self.binning = torch.empty(self.nb, dtype=torch.uint8, device=dev)
        self.pinned = torch.zeros(16, dtype=torch.int32).pin_memory()

    def frame(self, mode, cam=None, scale_modifier=1.0, sync_free=False, want_keys=False):
        """-> dict(color, ranges [T,2] int64, order [T] int64, R).  sync_free: gsr_forward with the capacity of __init__
        into the shared binning workspace; otherwise the two calls with a binning workspace of the frame's own size."""
        from gpu_util import product_settings
        from mvs_gaussian_splatting_amd import _lib
        from mvs_gaussian_splatting_amd.rasterizer import _make_params
        lib, dev, W, H, m = self.lib, self.dev, self.W, self.H, self.model
        e = torch.empty(0, device=dev)
        with torch.cuda.device(dev), torch.no_grad():
            stream = torch.cuda.current_stream(dev).cuda_stream
            st = product_settings(cam or self.cam, self.bg, 1, dev, scale_modifier=scale_modifier)
            params, keep = _make_params(dev, st, m.get_xyz.contiguous(), m.get_features.contiguous(), e,
                                        m.get_opacity.contiguous(), m.get_scaling.contiguous(),
                                        m.get_rotation.contiguous(), e)
            params.binning_mode = mode
            radii = torch.zeros(P, dtype=torch.int32, device=dev)
            color = torch.empty(3, H, W, device=dev)
            self.img[self.order_off:self.order_off + 4 * self.T] = 0xA5      # a tile order nobody wrote shows
            if sync_free:
                params.counts_pinned = self.pinned.data_ptr()
                _lib.check(lib.gsr_forward(C.byref(params), self.geom.data_ptr(), self.binning.data_ptr(), self.nb, self.cap,
                                           self.img.data_ptr(), radii.data_ptr(), color.data_ptr(), None, stream), "gsr_forward")
                torch.cuda.synchronize(dev)
                R, V = int(self.pinned[0]) & 0xffffffff, int(self.pinned[1]) & 0xffffffff
                assert R <= self.cap
                binning, lay = self.binning, (self.cap, P)
            else:
                R, V = C.c_uint32(0), C.c_uint32(0)
                _lib.check(lib.gsr_forward_preprocess(C.byref(params), self.geom.data_ptr(), radii.data_ptr(), stream,
                                                      C.byref(R), C.byref(V)), "pre")
                R, V = int(R.value), int(V.value)
                nb = lib.gsr_binning_bytes(R, V, W, H, mode)
                binning = torch.empty(max(nb, 256), dtype=torch.uint8, device=dev)
                _lib.check(lib.gsr_forward_render(C.byref(params), self.geom.data_ptr(), binning.data_ptr(), nb,
                                                  self.img.data_ptr(), R, V, color.data_ptr(), stream), "render")
                lay = (R, V)
            final_T = torch.empty(H, W, device=dev)
            n_contrib = torch.empty(H, W, dtype=torch.int32, device=dev)
            ranges = torch.empty(self.T, 2, dtype=torch.int32, device=dev)
            _lib.check(lib.gsr_debug_read_image(self.img.data_ptr(), W, H, final_T.data_ptr(), n_contrib.data_ptr(),
                                                ranges.data_ptr(), stream), "read_img")
            out = {"R": R}
            if want_keys and R > 0:
                keys = torch.empty(lay[0], dtype=torch.int64, device=dev)
                plist = torch.empty(lay[0], dtype=torch.int32, device=dev)
                _lib.check(lib.gsr_debug_read_binning(self.geom.data_ptr(), P, binning.data_ptr(), lay[0], lay[1], W, H, mode,
                                                      keys.data_ptr(), plist.data_ptr(), stream), "read_bin")
                out["keys"] = keys[:R].cpu().numpy().view(np.uint64)
            torch.cuda.synchronize(dev)
            order = self.img[self.order_off:self.order_off + 4 * self.T].view(torch.int32)
            out.update(color=color.cpu(), ranges=ranges.cpu().numpy().view(np.uint32).astype(np.int64),
                       order=order.cpu().numpy().view(np.uint32).astype(np.int64))
        del keep
        return out


def _away_camera(cam, dev):
    """The camera of ``cam`` turned by 180 degrees about the vertical axis: every Gaussian of the cloud lies behind it."""
    from mvs_gaussian_splatting_amd.synthetic import SyntheticCamera
    f = lambda fov, px: px / (2.0 * math.tan(fov * 0.5))  # noqa: E731
    return SyntheticCamera(cam.image_width, cam.image_height, f(cam.FoVx, cam.image_width), f(cam.FoVy, cam.image_height),
                           R=np.diag([-1.0, 1.0, -1.0]), T=np.zeros(3), device=dev)


def _assert_order(order, ranges, chunk, what):
    bucket = len_bucket(ranges[:, 1] - ranges[:, 0])
    T = ranges.shape[0]
    for c0 in range(0, T, chunk):
        c1 = min(c0 + chunk, T)
        o = order[c0:c1]
        assert np.array_equal(np.sort(o), np.arange(c0, c1)), f"{what}: tile order of chunk {c0} is no permutation"
        assert (np.diff(bucket[o]) <= 0).all(), f"{what}: length bucket increases along the order of chunk {c0}"
    assert np.array_equal(np.sort(order), np.arange(T)), f"{what}: tile order is no permutation of 0..T-1"


def _assert_fused_equals_keys64(got, ref, what):
    bad = np.nonzero((got["ranges"] != ref["ranges"]).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} ranges differ from the 64-bit key mode, first tile {bad[0]}: "
                           f"{got['ranges'][bad[0]]} vs {ref['ranges'][bad[0]]}")
    assert got["R"] == ref["R"]
    assert torch.equal(got["color"], ref["color"]), f"{what}: image differs from the 64-bit key mode"
    _assert_order(got["order"], got["ranges"], RIDER_CHUNK, what)


# 352 x 208 = 286 tiles: one pass; 640 x 400 = 1000 tiles: two passes, the last one segmented; 1000 x 600 = 63 x 38 = 2394
# tiles: no multiple of 8 nor of the rider's chunk; 2048 x 1024 = 8192 tiles: two rider chunks
SIZES = [(352, 208), (640, 400), (1000, 600), (2048, 1024)]


@pytest.fixture(scope="module")
def frames_1000(gpu_device):
    """The 1000-tile frame in both modes, shared by the tests that need it (nothing writes to it)."""
    from mvs_gaussian_splatting_amd import _lib
    f = _Frames(gpu_device, 640, 400)
    return f.frame(_lib.BINNING_TWO_LEVEL), f.frame(_lib.BINNING_KEYS64, want_keys=True)


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_ranges_and_image_equal_the_64_bit_key_mode(gpu_device, size, frames_1000):
    from mvs_gaussian_splatting_amd import _lib
    W, H = size
    assert SORT_THREADS == 512 and RIDER_CHUNK == 4096
    if size == (640, 400):
        got, ref = frames_1000
    else:
        f = _Frames(gpu_device, W, H)
        got, ref = f.frame(_lib.BINNING_TWO_LEVEL), f.frame(_lib.BINNING_KEYS64)
    T = ((W + 15) // 16) * ((H + 15) // 16)
    assert T == {(352, 208): 286, (640, 400): 1000, (1000, 600): 2394, (2048, 1024): 8192}[size]
    assert ref["R"] > 1000 and (ref["ranges"][:, 1] > ref["ranges"][:, 0]).sum() > T // 8
    _assert_fused_equals_keys64(got, ref, f"{W}x{H}")
    _assert_order(ref["order"], ref["ranges"], 8192, f"{W}x{H} keys64")      # build_tile_order_kernel: chunks of 8192


@pytest.mark.parametrize("size", [(352, 208), (640, 400)], ids=["one_pass", "two_passes"])
def test_frame_without_instances_between_ordinary_frames(gpu_device, size):
    """gsr_forward three times into the same workspaces: an ordinary view, the camera turned away (R = 0: the scattering
    blocks all exit on the device-side count, the rider must not), the ordinary view again."""
    from mvs_gaussian_splatting_amd import _lib
    W, H = size
    f = _Frames(gpu_device, W, H, cap=1 << 19)
    ref = f.frame(_lib.BINNING_KEYS64)
    first = f.frame(_lib.BINNING_TWO_LEVEL, sync_free=True)
    _assert_fused_equals_keys64(first, ref, "first frame")
    empty = f.frame(_lib.BINNING_TWO_LEVEL, cam=_away_camera(f.cam, gpu_device), sync_free=True)
    assert empty["R"] == 0
    assert not empty["ranges"].any(), "frame without instances: a range is not (0, 0)"
    assert torch.equal(empty["color"], f.bg.cpu()[:, None, None].expand(3, H, W))
    _assert_order(empty["order"], empty["ranges"], RIDER_CHUNK, "frame without instances")
    third = f.frame(_lib.BINNING_TWO_LEVEL, sync_free=True)
    assert np.array_equal(third["ranges"], first["ranges"]) and torch.equal(third["color"], first["color"])
    _assert_order(third["order"], third["ranges"], RIDER_CHUNK, "third frame")


def test_capacity_path_frame_below_the_learnt_capacity(gpu_device):
    """The capacity is the instance count of a heavier frame (scale modifier 1); the lighter frame (0.5) goes through
    gsr_forward with a scatter grid sized for that capacity and its count in device memory."""
    from mvs_gaussian_splatting_amd import _lib
    W, H = 1000, 600
    probe = _Frames(gpu_device, W, H)
    heavy_ref = probe.frame(_lib.BINNING_KEYS64)
    light_ref = probe.frame(_lib.BINNING_KEYS64, scale_modifier=0.5)
    assert 1000 < light_ref["R"] < heavy_ref["R"] - 4096, "the lighter frame should leave whole sort blocks unused"
    f = _Frames(gpu_device, W, H, cap=heavy_ref["R"])
    heavy = f.frame(_lib.BINNING_TWO_LEVEL, sync_free=True)
    _assert_fused_equals_keys64(heavy, heavy_ref, "heavy frame at capacity")
    light = f.frame(_lib.BINNING_TWO_LEVEL, scale_modifier=0.5, sync_free=True)
    _assert_fused_equals_keys64(light, light_ref, "light frame below capacity")


def test_raw_tile_sort_entry_gives_the_fused_paths_ranges(gpu_device, frames_1000):
    """gsr_sort_tile_runs_u32 still runs the stand-alone kernel (1024 lanes) behind the sort: on the tile ids of the
    1000-tile frame it must give the ranges the rider gave."""
    from mvs_gaussian_splatting_amd import _lib
    lib, dev = _lib.load(), gpu_device
    got, ref = frames_1000
    tiles = (ref["keys"] >> np.uint64(32)).astype(np.uint32)
    n, n_keys = tiles.shape[0], 1000
    tiles = tiles[np.random.default_rng(7).permutation(n)]
    k = torch.from_numpy(tiles.view(np.int32)).to(dev)
    v = torch.arange(n, dtype=torch.int32, device=dev)
    kt, vt = torch.empty_like(k), torch.empty_like(v)
    ranges = torch.empty(n_keys, 2, dtype=torch.int32, device=dev)
    order = torch.empty(n_keys, dtype=torch.int32, device=dev)
    scratch = torch.empty(lib.gsr_sort_scratch_bytes(n), dtype=torch.uint8, device=dev)
    in_tmp, valid = C.c_int32(-1), C.c_int32(-1)
    assert ranges.data_ptr() % 16 == 0
    with torch.cuda.device(dev):
        _lib.check(lib.gsr_sort_tile_runs_u32(k.data_ptr(), v.data_ptr(), kt.data_ptr(), vt.data_ptr(), n, None, 10, n_keys,
                                              ranges.data_ptr(), order.data_ptr(), scratch.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream, C.byref(in_tmp), C.byref(valid)),
                   "gsr_sort_tile_runs_u32")
        torch.cuda.synchronize()
    assert valid.value == 1
    raw = ranges.cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(raw, got["ranges"])
    _assert_order(order.cpu().numpy().view(np.uint32).astype(np.int64), raw, 8192, "raw entry")
