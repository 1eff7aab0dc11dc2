"""Times the load-time image ingest: ``image_ingest.load_image`` (HIP kernels) against ``load_image_host`` (numpy, Pillow,
torch on the CPU) in one process, stage by stage and chained, on the two shapes scene loading meets:

  * a 4946x3286 RGB photograph resized to 1600 pixels wide (the ``-r -1`` rule on a full-size COLMAP image);
  * an 800x800 RGBA Blender frame composited over white (no resize).

Device stages are timed with device events after a warm-up, the median of ``--repeats`` runs.  The chained device figure
is wall-clock time up to a device synchronise: it includes the host-to-device copy of the decoded bytes and the host's
share (table look-up, launches), which device events would leave out.  The file decode (Pillow) is outside every figure: it is the same
on both paths.  Prints one JSON line.

    python tools/bench_ingest.py [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvs_gaussian_splatting_amd import image_ingest as ii  # noqa: E402
from mvs_gaussian_splatting_amd.scene import load_resolution  # noqa: E402


def device_ms(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def host_ms(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t))
    return statistics.median(out)


def synced_ms(fn, repeats):
    def run():
        fn()
        torch.cuda.synchronize()
    return host_ms(run, repeats, warmup=3)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args(argv)
    from PIL import Image
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    n = args.repeats
    result = {"tool": "bench_ingest", "repeats": n, "device": torch.cuda.get_device_name(0), "unit": "ms (median)"}

    photo = rng.integers(0, 256, (3286, 4946, 3), dtype=np.uint8)
    size = load_resolution(4946, 3286, -1)
    photo_dev = torch.from_numpy(photo).to(dev)
    small_dev = ii.resize_u8(photo_dev, size)
    small = small_dev.cpu().numpy()
    pil = Image.fromarray(photo)
    exact = bool(torch.equal(ii.load_image(photo, size, dev).cpu(), ii.load_image_host(photo, size)))
    result["photo_4946x3286_to_%dx%d" % size] = {
        "bit_equal": exact,
        "gpu": {"resize": device_ms(lambda: ii.resize_u8(photo_dev, size), n),
                "to_float": device_ms(lambda: ii.to_float_chw(small_dev), n),
                "tables_host": host_ms(lambda: (ii.resize_tables(4946, size[0]), ii.resize_tables(3286, size[1])), n),
                "chain_with_upload": synced_ms(lambda: ii.load_image(photo, size, dev), n)},
        "host": {"resize": host_ms(lambda: np.array(pil.resize(size)), n),
                 "to_float": host_ms(lambda: ii.to_float_host(small), n),
                 "chain": host_ms(lambda: ii.load_image_host(photo, size), n)}}

    frame = rng.integers(0, 256, (800, 800, 4), dtype=np.uint8)
    frame_dev = torch.from_numpy(frame).to(dev)
    bg = [1, 1, 1]
    rgb_dev = ii.composite_u8(frame_dev, bg)
    rgb = rgb_dev.cpu().numpy()
    exact = bool(torch.equal(ii.load_image(frame, (800, 800), dev, bg).cpu(), ii.load_image_host(frame, (800, 800), bg)))
    result["blender_800x800_rgba"] = {
        "bit_equal": exact,
        "gpu": {"composite": device_ms(lambda: ii.composite_u8(frame_dev, bg), n),
                "to_float": device_ms(lambda: ii.to_float_chw(rgb_dev), n),
                "chain_with_upload": synced_ms(lambda: ii.load_image(frame, (800, 800), dev, bg), n)},
        "host": {"composite": host_ms(lambda: ii.composite_host(frame, np.array(bg)), n),
                 "to_float": host_ms(lambda: ii.to_float_host(rgb), n),
                 "chain": host_ms(lambda: ii.load_image_host(frame, (800, 800), bg), n)}}
    for v in list(result.values()):
        if isinstance(v, dict):
            v["images_per_s"] = {"gpu": 1e3 / v["gpu"]["chain_with_upload"], "host": 1e3 / v["host"]["chain"]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
