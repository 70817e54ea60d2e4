"""Image explainers and SuperpixelTransformer with the device path on against
off, at the same commit.

    python tools/image_explain_bench.py                    # on an MI355X
    python tools/image_explain_bench.py --out profiles/image_explain_bench.txt
    rocprofv3 --kernel-trace --stats -- \\
        python tools/image_explain_bench.py --trace-run    # launches only

Both paths of a pair are warmed up, then alternated in one process, five
samples each; a sample is a host clock around one transform, which ends in
device-to-host copies of the scores and the host fit.  Medians, min-max:
  (a) ImageLIME, one 224 x 224 x 3 uint8 image, ImageFeaturizer(ResNet50),
      cellSize 16, 512 samples (the default)
  (b) ImageSHAP, the same, 2048 samples (the default for m = 196)
  (c) SuperpixelTransformer over a column of 256 such images with device
      "cuda"; the host path ("cpu") over the column's first 8, per image
For (a) and (b) the split of one explained image between segmentation, sample
building and the model's forward is timed on both paths, each part ending in
a device synchronise.  The trace run calls backend.slic_segment (the 256-image
column) and backend.masked_image_batch (512 and 2050 samples) alone, 4 calls
each.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mmlspark_amd.explainers.lime import (ImageLIME,  # noqa: E402
                                          SuperpixelTransformer)
from mmlspark_amd.explainers.sampler import (ImageSampler,  # noqa: E402
                                             lime_sample_states,
                                             slic_superpixels)
from mmlspark_amd.explainers.shap import ImageSHAP  # noqa: E402
from mmlspark_amd.models.image_featurizer import (ImageFeaturizer,  # noqa: E402
                                                  _unit_lut)
from mmlspark_amd.ops import backend  # noqa: E402

_OUT = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if _OUT is not None:
        _OUT.write(line + "\n")
        _OUT.flush()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def summary(name, samples):
    row = {"what": name, "median_s": round(statistics.median(samples), 5),
           "min_s": round(min(samples), 5), "max_s": round(max(samples), 5),
           "samples": len(samples)}
    emit(row)
    return row


def pair(name, off, on, df, compare, n_samples=5):
    a, b = off.transform(df), on.transform(df)
    emit(dict({"what": name + ": device path vs host path"}, **compare(a, b)))
    ta, tb = [], []
    for _ in range(n_samples):
        for ex, acc in ((off, ta), (on, tb)):
            acc.append(timed(lambda: ex.transform(df))[0])
    ra, rb = summary(name + ", host path", ta), summary(name + ", device path", tb)
    emit({"what": name + ": host/device at the medians",
          "value": round(ra["median_s"] / rb["median_s"], 3),
          "ranges_overlap": not (min(ta) > max(tb) or min(tb) > max(ta))})


def split(name, model, img, n, n_samples=5):
    """Per explained image: segmentation, sample building, model forward."""
    dev = torch.device("cuda")
    parts = {k: [] for k in ("host segmentation", "host sample building",
                             "host-path forward (rows to batch, upload, model)",
                             "device segmentation (upload included)",
                             "device sample building (pack, upload, kernel)",
                             "device-path forward (model)")}
    segments = slic_superpixels(img, 16, 10.0)
    m = int(segments.max()) + 1
    states = lime_sample_states(m, n, np.random.default_rng(0))
    for _ in range(n_samples + 1):          # the first round warms up
        t, _ = timed(lambda: slic_superpixels(img, 16, 10.0))
        parts["host segmentation"].append(t)
        t, imgs = timed(lambda: ImageSampler(img, segments).apply(states))
        parts["host sample building"].append(t)
        t, _ = timed(lambda: model.transform(pd.DataFrame({"image": imgs})))
        parts["host-path forward (rows to batch, upload, model)"].append(t)
        t, (dimg, seg) = timed(lambda: (
            lambda d: (d, backend.slic_segment([d], 16, 10.0)[0][0]))(
                torch.from_numpy(img).to(dev)))
        parts["device segmentation (upload included)"].append(t)
        t, batch = timed(lambda: backend.masked_image_batch(
            dimg, seg, backend.pack_states(states).to(dev), 0,
            model.image_input_size(img.shape), _unit_lut(dev), m=m))
        parts["device sample building (pack, upload, kernel)"].append(t)
        t, _ = timed(lambda: model.score_image_batch(batch))
        parts["device-path forward (model)"].append(t)
    for k, v in parts.items():
        summary("%s, %d samples: %s" % (name, n, k), v[1:])


def trace_run(imgs):
    dev = torch.device("cuda")
    col = [torch.from_numpy(a).to(dev) for a in imgs]
    for _ in range(4):
        labels, _ = backend.slic_segment(col, 16, 10.0)
    m = int(labels[0].max()) + 1
    for n in (512, 2050):
        st = backend.pack_states(lime_sample_states(
            m, n, np.random.default_rng(0))).to(dev)
        for _ in range(4):
            backend.masked_image_batch(col[0], labels[0], st, 0, 224,
                                       _unit_lut(dev), m=m)
    torch.cuda.synchronize()
    emit({"what": "trace run, 4 calls each in trace order",
          "slic_segment": "%d images 224x224x3, cell 16, 5 iterations: 1 "
          "seed + 5 assign + 5 update launches a call" % len(col),
          "masked_image_batch": "224x224x3 -> (n, 3, 224, 224), n = 512 then "
          "2050, m = %d" % m,
          "output_bytes_per_call": [n * 3 * 224 * 224 * 4 for n in (512, 2050)]})


def main():
    global _OUT
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--column", type=int, default=256)
    ap.add_argument("--host-images", type=int, default=8)
    ap.add_argument("--out", default=None, help="also append rows to a file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs a GPU: a CPU timing says nothing about these paths")
    if args.out:
        _OUT = open(args.out, "a")
    rng = np.random.default_rng(0)
    # smooth colour fields plus noise: superpixels with structure to follow
    yy, xx = np.mgrid[0:224, 0:224]
    imgs = []
    for i in range(args.column):
        base = 127 + 100 * np.sin((yy * (1 + i % 5) + xx * (2 + i % 3)) / 40.0)
        a = base[..., None] + rng.normal(0, 12, size=(224, 224, 3))
        imgs.append(np.clip(a, 0, 255).astype(np.uint8))
    if args.trace_run:
        trace_run(imgs)
        return
    torch.manual_seed(0)
    model = ImageFeaturizer(modelName="ResNet50", inputCol="image",
                            outputCol="features", device="cuda")
    one = pd.DataFrame({"image": imgs[:1]})

    def explained(a, b):
        ea, eb = a["explanation"][0], b["explanation"][0]
        return {"superpixels_equal": bool(np.array_equal(
                    a["superpixels"][0], b["superpixels"][0])),
                "max_abs_diff": float(np.abs(ea - eb).max()),
                "max_abs_value": float(np.abs(ea).max())}

    for name, cls, n in (("(a) ImageLIME 224x224, ResNet50, 512 samples",
                          ImageLIME, 512),
                         ("(b) ImageSHAP 224x224, ResNet50, 2048 samples",
                          ImageSHAP, 2050)):
        kw = dict(model=model, inputCol="image", targetCol="features",
                  targetClasses=[0])
        pair(name, cls(fusedSampling=False, **kw), cls(fusedSampling=True, **kw),
             one, explained)
        split(name, model, imgs[0], n)
    # (c): the device path over the whole column; the host path costs seconds
    # an image, so it is timed over the column's first --host-images images
    # in the same alternated session and both are reported per image
    col = pd.DataFrame({"image": imgs})
    head = col.head(args.host_images)
    off = SuperpixelTransformer(inputCol="image")
    on = SuperpixelTransformer(inputCol="image", device="cuda")
    a, b = off.transform(head), on.transform(col)
    emit({"what": "(c) SuperpixelTransformer: device labels vs host labels, "
          "first %d images" % len(head),
          "label_mismatch_fraction": float(np.mean([
              np.mean(x != y) for x, y in zip(a["superpixels"],
                                              b["superpixels"])]))})
    ta, tb = [], []
    for _ in range(3):
        ta.append(timed(lambda: off.transform(head))[0] / len(head))
        tb.append(timed(lambda: on.transform(col))[0] / len(col))
    ra = summary("(c) SuperpixelTransformer host path, per image (%d images)"
                 % len(head), ta)
    rb = summary("(c) SuperpixelTransformer device path, per image (%d "
                 "images)" % len(col), tb)
    emit({"what": "(c) host/device per image at the medians",
          "value": round(ra["median_s"] / rb["median_s"], 1),
          "ranges_overlap": not (min(ta) > max(tb) or min(tb) > max(ta))})


if __name__ == "__main__":
    main()
