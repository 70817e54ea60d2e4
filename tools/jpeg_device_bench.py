"""Host path vs device path for JPEG ingestion, at the same commit.

    python tools/jpeg_device_bench.py --host-only     # no GPU needed
    python tools/jpeg_device_bench.py                 # on an MI355X
    rocprofv3 --kernel-trace --stats -- \\
        python tools/jpeg_device_bench.py --trace-run # 8 device batches only

Host-only mode times `decode_jpeg` (entropy decode + reconstruction) against
`decode_jpeg_coefficients` (entropy decode + export) on one thread.  The
difference is the share of today's decode time that the device path can
remove; the rest is Huffman decoding and stays on the host.

GPU mode alternates the two paths, five samples each after warm-up, every
sample ended by a device synchronise, and prints median and min-max:
  bytes -> uint8 device batch   (a) thread-pool decode + np.stack + H2D
                                (b) decode_jpeg_batch
  bytes -> ResNet-50 features   decodeOnDevice off / on
The images are the 224x224 q90 set of bench_image.py --bytes-to-features.
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mmlspark_amd.io_http import _jpeg_native  # noqa: E402
from mmlspark_amd.io_http.jpeg_codec import encode_jpeg  # noqa: E402


def make_blobs(n):
    """bench_image.py's images: 16 distinct 224x224 q90 streams, cycled."""
    rng = np.random.default_rng(0)
    side = 224
    yy, xx = np.mgrid[0:side, 0:side]
    base = (np.sin(xx / 9.0) * np.cos(yy / 13.0) * 90 + 128)
    imgs = []
    for i in range(16):
        img = np.clip(np.stack([np.roll(base, i, 0)] * 3, -1)
                      + rng.normal(0, 8, (side, side, 3)), 0, 255)
        imgs.append(encode_jpeg(img.astype(np.uint8), quality=90))
    return [imgs[i % 16] for i in range(n)]


def summary(name, samples, n_images):
    med = statistics.median(samples)
    row = {"what": name, "median_s": round(med, 5),
           "min_s": round(min(samples), 5), "max_s": round(max(samples), 5),
           "images_per_s_at_median": round(n_images / med, 1),
           "samples": len(samples)}
    print(json.dumps(row), flush=True)
    return row


def host_only(args):
    blobs = make_blobs(16)
    reps = args.reps

    def run(fn):
        out = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(reps):
                for b in blobs:
                    fn(b)
            out.append((time.perf_counter() - t0) / (reps * len(blobs)))
        return out

    run(_jpeg_native.decode_jpeg)  # warm caches
    full = run(_jpeg_native.decode_jpeg)
    ent = run(_jpeg_native.decode_jpeg_coefficients)
    f, e = statistics.median(full), statistics.median(ent)
    print(json.dumps({
        "what": "CPU timing of host code, one thread, 224x224 q90",
        "decode_jpeg_ms": round(f * 1e3, 4),
        "decode_jpeg_ms_min_max": [round(min(full) * 1e3, 4),
                                   round(max(full) * 1e3, 4)],
        "decode_jpeg_coefficients_ms": round(e * 1e3, 4),
        "decode_jpeg_coefficients_ms_min_max": [round(min(ent) * 1e3, 4),
                                                round(max(ent) * 1e3, 4)],
        "entropy_share_of_decode": round(e / f, 4),
        "ceiling_speedup_of_decode": round(f / e, 3),
    }), flush=True)


def host_batch(blobs, pool, device):
    dec = list(pool.map(lambda b: _jpeg_native.decode_jpeg(b).numpy(), blobs))
    return torch.from_numpy(np.stack(dec)).to(device)


def device_batch(blobs, device):
    from mmlspark_amd.io_http.jpeg_device import decode_jpeg_batch
    return torch.stack(decode_jpeg_batch(blobs, device, num_threads=16))


def alternate(fa, fb, n_samples=5):
    a, b = [], []
    for _ in range(n_samples):
        for fn, acc in ((fa, a), (fb, b)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append(time.perf_counter() - t0)
    return a, b


def gpu(args):
    import pandas as pd
    from mmlspark_amd.models.image_featurizer import ImageFeaturizer
    device = torch.device("cuda")
    blobs = make_blobs(args.images)
    bs = 256
    if args.trace_run:
        for _ in range(8):
            device_batch(blobs[:bs], device)
        torch.cuda.synchronize()
        return
    with ThreadPoolExecutor(max_workers=16) as pool:
        def run_host():
            for s in range(0, len(blobs), bs):
                host_batch(blobs[s:s + bs], pool, device)

        def run_dev():
            for s in range(0, len(blobs), bs):
                device_batch(blobs[s:s + bs], device)

        # same pixels before any timing is believed
        h = host_batch(blobs[:32], pool, device)
        d = device_batch(blobs[:32], device)
        diff = (h.int() - d.int()).abs()
        print(json.dumps({"what": "device vs host pixels, 32 images",
                          "max_abs_diff": int(diff.max()),
                          "differing": int((diff != 0).sum()),
                          "samples": diff.numel()}), flush=True)
        run_host(); run_dev()
        torch.cuda.synchronize()
        a, b = alternate(run_host, run_dev)
    ra = summary("bytes->uint8 device batch, host path (a)", a, len(blobs))
    rb = summary("bytes->uint8 device batch, decode_jpeg_batch (b)", b,
                 len(blobs))
    print(json.dumps({"what": "speed-up (a)/(b) at the medians",
                      "value": round(ra["median_s"] / rb["median_s"], 3)}),
          flush=True)
    if args.no_features:
        return
    df = pd.DataFrame({"image": blobs})
    off = ImageFeaturizer(modelName="ResNet50", cutOutputLayers=1,
                          imageSize=224, device="cuda")
    on = ImageFeaturizer(modelName="ResNet50", cutOutputLayers=1,
                         imageSize=224, device="cuda",
                         decodeOnDevice=True).setModel(off.module)
    warm = pd.DataFrame({"image": blobs[:2 * bs]})
    off.transform(warm); on.transform(warm)
    torch.cuda.synchronize()
    a, b = alternate(lambda: off.transform(df), lambda: on.transform(df))
    ra = summary("bytes->features ResNet-50, decodeOnDevice=False", a,
                 len(blobs))
    rb = summary("bytes->features ResNet-50, decodeOnDevice=True", b,
                 len(blobs))
    print(json.dumps({"what": "speed-up off/on at the medians",
                      "value": round(ra["median_s"] / rb["median_s"], 3)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--trace-run", action="store_true",
                    help="8 device batches of 256 and exit (for a kernel "
                         "trace)")
    ap.add_argument("--no-features", action="store_true")
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=4)
    args = ap.parse_args()
    if args.host_only:
        host_only(args)
    else:
        if not torch.cuda.is_available():
            sys.exit("GPU mode needs a GPU; use --host-only without one")
        gpu(args)


if __name__ == "__main__":
    main()
