"""A numpy restatement of the device's two-pass integer resize (``csrc/image.hip``): the same tables, the same
accumulator, one output index at a time.  It lets the host tests pin ``image_ingest.resize_tables`` and the pass
arithmetic to Pillow byte for byte without a GPU."""
import numpy as np

from mvs_gaussian_splatting_amd.image_ingest import PRECISION_BITS, resize_tables


def resize_pass(img: np.ndarray, out_len: int, axis: int) -> np.ndarray:
    """One pass along ``axis`` (0: vertical, 1: horizontal) of an ``[H, W, C]`` uint8 image."""
    a = np.moveaxis(img, axis, 0).astype(np.int32)
    bounds, taps = resize_tables(a.shape[0], out_len)
    out = np.empty((out_len,) + a.shape[1:], np.uint8)
    for o in range(out_len):
        first, count = int(bounds[o, 0]), int(bounds[o, 1])
        acc = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), np.int32)
        for j in range(count):
            acc += a[first + j] * taps[o, j]
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img: np.ndarray, size) -> np.ndarray:
    """``Image.resize(size)`` for ``[H, W, C]`` uint8, C = 1 or 3: horizontal pass, then vertical; equal sizes skip."""
    out_w, out_h = int(size[0]), int(size[1])
    if out_w != img.shape[1]:
        img = resize_pass(img, out_w, 1)
    if out_h != img.shape[0]:
        img = resize_pass(img, out_h, 0)
    return np.ascontiguousarray(img)
