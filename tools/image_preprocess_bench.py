"""Fused image preprocessing against the parent paths, at the same commit.

    python tools/image_preprocess_bench.py                 # on an MI355X
    python tools/image_preprocess_bench.py --out profiles/image_preprocess_bench.txt
    rocprofv3 --kernel-trace --stats -- \\
        python tools/image_preprocess_bench.py --trace-run # launches only

Both paths of a pair are warmed up, then alternated in one process, five
samples each; every sample is a host clock around a call that ends in a
device-to-host copy or a synchronise.  Medians with min-max:
  (a) ImageTransformer resize 224x224 + normalize, uniform 256x256 uint8
      images: fused=True against today's batched torch path
  (b) the same stages on sizes drawn from 160..512: fused=True against
      today's per-image CPU loop
  (c) JPEG bytes -> ResNet-50 features, decodeOnDevice=True, batch 256:
      fusedPreprocess on against off, on mixed sizes and on the uniform
      224x224 set of tools/jpeg_device_bench.py
The trace run launches image_preprocess_k alone on the batches of (a), (b)
and (c) and prints the bytes each launch has to move, for the bytes/s figure.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mmlspark_amd.io_http.jpeg_codec import encode_jpeg  # noqa: E402
from mmlspark_amd.models.images import (ImageTransformer,  # noqa: E402
                                        compile_image_plan)
from mmlspark_amd.ops import backend  # noqa: E402

_OUT = None
STAGES = [{"op": "resize", "height": 224, "width": 224},
          {"op": "normalize", "mean": [0.485, 0.456, 0.406],
           "std": [0.229, 0.224, 0.225]}]


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if _OUT is not None:
        _OUT.write(line + "\n")
        _OUT.flush()


def summary(name, samples, n_images):
    med = statistics.median(samples)
    row = {"what": name, "median_s": round(med, 5),
           "min_s": round(min(samples), 5), "max_s": round(max(samples), 5),
           "images_per_s_at_median": round(n_images / med, 1),
           "samples": len(samples)}
    emit(row)
    return row


def alternate(fa, fb, n_samples=5):
    a, b = [], []
    for _ in range(n_samples):
        for fn, acc in ((fa, a), (fb, b)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            acc.append(time.perf_counter() - t0)
    return a, b


def pair(name, parent, fused, n_images):
    parent(); fused()
    torch.cuda.synchronize()
    a, b = alternate(parent, fused)
    ra = summary(name + ", parent path", a, n_images)
    rb = summary(name + ", fused", b, n_images)
    emit({"what": name + ": parent/fused at the medians",
          "value": round(ra["median_s"] / rb["median_s"], 3),
          "ranges_overlap": not (min(a) > max(b) or min(b) > max(a))})


def uniform_images(n):
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, size=(16, 256, 256, 3), dtype=np.uint8)
    return [base[i % 16] for i in range(n)]


def mixed_images(n):
    rng = np.random.default_rng(1)
    base = [rng.integers(0, 256, size=(int(h), int(w), 3), dtype=np.uint8)
            for h, w in rng.integers(160, 513, size=(32, 2))]
    return [base[i % 32] for i in range(n)]


def smooth_image(h, w, i, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.sin(xx / 9.0) * np.cos(yy / 13.0) * 90 + 128
    img = np.clip(np.stack([np.roll(base, i, 0)] * 3, -1)
                  + rng.normal(0, 8, (h, w, 3)), 0, 255)
    return img.astype(np.uint8)


def jpeg_blobs(n, mixed, cache=None):
    """16 distinct q90 streams, cycled: 224x224 (jpeg_device_bench.py's
    set) or sizes drawn from 160..512.  `cache` names a directory that keeps
    the encoded streams between runs (the encoder is host Python)."""
    path = cache and os.path.join(
        cache, "image_preprocess_bench_%s.npy" % ("mixed" if mixed else "224"))
    if path and os.path.exists(path):
        blobs = [bytes(b) for b in np.load(path, allow_pickle=True)]
    else:
        rng = np.random.default_rng(0)
        sizes = rng.integers(160, 513, size=(16, 2)) if mixed \
            else np.full((16, 2), 224)
        blobs = [encode_jpeg(smooth_image(int(h), int(w), i, rng), quality=90)
                 for i, (h, w) in enumerate(sizes)]
        if path:
            os.makedirs(cache, exist_ok=True)
            np.save(path, np.array(blobs, dtype=object), allow_pickle=True)
    return [blobs[i % 16] for i in range(n)]


def transformer_pair(name, imgs):
    import pandas as pd
    df = pd.DataFrame({"image": imgs})
    parent = ImageTransformer(stages=STAGES)
    fused = ImageTransformer(stages=STAGES, fused=True)
    a = parent.transform(df.iloc[:64])["out_image"]
    b = fused.transform(df.iloc[:64])["out_image"]
    worst = max(float(np.abs(x - y).max()) for x, y in zip(a, b))
    emit({"what": name + ": fused vs parent values, 64 images",
          "max_abs_diff": worst})
    pair(name, lambda: parent.transform(df), lambda: fused.transform(df),
         len(imgs))


def featurizer_pair(name, blobs):
    import pandas as pd
    from mmlspark_amd.models.image_featurizer import ImageFeaturizer
    df = pd.DataFrame({"image": blobs})
    off = ImageFeaturizer(modelName="ResNet50", cutOutputLayers=1,
                          imageSize=224, device="cuda", decodeOnDevice=True)
    on = ImageFeaturizer(modelName="ResNet50", cutOutputLayers=1,
                         imageSize=224, device="cuda", decodeOnDevice=True,
                         fusedPreprocess=True).setModel(off.module)
    a = off._coerce(np.array(blobs[:32], dtype=object))
    b = on._coerce(np.array(blobs[:32], dtype=object))
    emit({"what": name + ": fused vs parent network input, 32 images",
          "max_abs_diff": float((a - b).abs().max())})
    pair(name, lambda: off.transform(df), lambda: on.transform(df),
         len(blobs))


def plan_bytes(plan):
    """Bytes one launch must move: every output sample written once, and of
    the source the smaller of the pre-window and the taps (4 per output
    pixel and source channel, 1 on the copy path)."""
    d = plan.idesc.numpy()
    isz = 1 if plan.src_dtype == torch.uint8 else 4
    osz = 1 if plan.out_dtype == torch.uint8 else 4
    taps = np.where(d[:, 8] & 16, 4, 1) * d[:, 13] * d[:, 14] * d[:, 3]
    window = d[:, 6] * d[:, 7] * d[:, 3]
    return int((np.minimum(taps, window) * isz).sum()), \
        int((d[:, 13] * d[:, 14] * d[:, 15] * osz).sum())


def trace_run(args):
    """image_preprocess_k alone, 8 launches per batch, for a kernel trace."""
    dev = torch.device("cuda")
    batches = [("uniform 256x256 -> 224x224 f32 HWC", uniform_images(256),
                "HWC"),
               ("mixed 160..512 -> 224x224 f32 HWC", mixed_images(256), "HWC"),
               ("mixed 160..512 -> 224x224 f32 CHW", mixed_images(256), "CHW")]
    for name, imgs, layout in batches:
        plan = compile_image_plan(STAGES, [im.shape for im in imgs],
                                  np.uint8, "float32", layout)
        src = torch.from_numpy(np.concatenate(
            [im.reshape(-1) for im in imgs])).to(dev)
        out = torch.empty(plan.out_numel, dtype=plan.out_dtype, device=dev)
        for _ in range(8):
            backend.image_preprocess(src, plan.idesc, plan.fdesc,
                                     plan.work_off, out)
        torch.cuda.synchronize()
        rd, wr = plan_bytes(plan)
        emit({"what": "trace batch, 8 launches in trace order", "batch": name,
              "images": len(imgs), "work_items": int(plan.work_off[-1]),
              "source_bytes_per_launch": rd, "output_bytes_per_launch": wr})


def main():
    global _OUT
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--mixed-images", type=int, default=1024)
    ap.add_argument("--no-features", action="store_true")
    ap.add_argument("--out", default=None, help="also append rows to a file")
    ap.add_argument("--blob-cache", default=None,
                    help="directory that keeps the encoded JPEG streams")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: a CPU timing says nothing about these paths")
    if args.out:
        _OUT = open(args.out, "a")
    if args.trace_run:
        trace_run(args)
        return
    transformer_pair("(a) ImageTransformer resize+normalize, %d uniform "
                     "256x256" % args.images, uniform_images(args.images))
    transformer_pair("(b) ImageTransformer resize+normalize, %d images of "
                     "160..512" % args.mixed_images,
                     mixed_images(args.mixed_images))
    if args.no_features:
        return
    featurizer_pair("(c) bytes->ResNet-50 features, mixed 160..512 q90, "
                    "batch 256, %d images" % args.mixed_images,
                    jpeg_blobs(args.mixed_images, True, args.blob_cache))
    featurizer_pair("(c) bytes->ResNet-50 features, uniform 224x224 q90, "
                    "batch 256, %d images" % args.images,
                    jpeg_blobs(args.images, False, args.blob_cache))


if __name__ == "__main__":
    main()
