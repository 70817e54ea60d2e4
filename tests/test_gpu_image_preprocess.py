"""image_preprocess_k on MI355X: the smallest shapes at which the kernel can
go wrong, alone and mixed in one launch.  Every comparison is bit-equality
with cpu_ref.image_preprocess (whose own correctness is
test_image_preprocess_ref.py's subject)."""
import itertools

import numpy as np
import pandas as pd
import pytest
import torch

from mmlspark_amd.io_http import jpeg_codec
from mmlspark_amd.ops import backend

from . import image_preprocess_cases as cases
from . import jpeg_device_cases as jcases
from .image_preprocess_cases import (color, crop, flip, normalize, resize,
                                     threshold)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")

FLIPS = [[], [flip(1)], [flip(0)], [flip(-1)]]


def _imgs(shapes, dtype, seed=0):
    rng = np.random.default_rng(seed)
    imgs = [cases.rand_image(rng, *s, dtype=dtype) for s in shapes]
    for im in imgs:             # samples exactly at and beside the thresholds
        n = min(3, im.size)
        im.reshape(-1)[:n] = (127, 128, 0)[:n]
    return imgs


def _groups(dtype):
    """[(stages, layout, images)] covering the shapes, geometry and pointwise
    ops of the contract for one source dtype.  The tile is 64 x 8 output
    pixels, 4 rows of threads taking two rows each."""
    g = []
    # tiny sources and outputs; up- and downscale; identity (copy path)
    g.append(([resize(3, 3)], "HWC",
              _imgs([(1, 1, 3), (1, 5, 1), (5, 1, 4), (7, 7, 3), (3, 3, 3)],
                    dtype, 1)))
    g.append(([resize(1, 1)], "CHW", _imgs([(1, 1, 1), (5, 1, 3), (4, 6, 4)],
                                           dtype, 2)))
    g.append(([resize(5, 5)], "HWC", _imgs([(2, 2, 3), (5, 5, 3)], dtype, 3)))
    # tile edges: widths 63 / 64 / 65, heights 3 / 4 / 5 / 7 / 8 / 9
    for k, (w, h) in enumerate(itertools.product((63, 64, 65),
                                                 (3, 4, 5, 7, 8, 9))):
        layout = "CHW" if k % 2 else "HWC"
        c = (1, 3, 4)[k % 3]
        g.append(([resize(h, w)], layout, _imgs([(6, 50, c)], dtype, 10 + k)))
        g.append(([], layout, _imgs([(h, w, c)], dtype, 40 + k)))
    # channel maps: gray, bgr2rgb, both, gray replicated to three
    for st in ([color("gray")], [color("bgr2rgb")],
               [color("bgr2rgb"), color("gray")], [color("_replicate3")]):
        g.append(([resize(6, 9)] + st, "CHW",
                  _imgs([(5, 4, 1), (5, 4, 3), (4, 7, 4)], dtype, 70)))
    # windows touching every edge, clipped by the edge, around a resize
    for pre, post in [(crop(0, 0, 4, 5), crop(0, 0, 3, 3)),
                      (crop(3, 2, 99, 99), crop(4, 5, 99, 99)),
                      (crop(0, 2, 99, 3), crop(1, 0, 2, 99))]:
        g.append(([pre, resize(8, 10), post], "HWC",
                  _imgs([(9, 11, 3), (6, 8, 3), (12, 7, 1)], dtype, 80)))
        g.append(([pre, post], "HWC", _imgs([(12, 14, 3), (9, 9, 3)], dtype,
                                            81)))
    # every flip combination before and after the resize
    for a, b in itertools.product(FLIPS, FLIPS):
        g.append((a + [crop(1, 0, 5, 6), resize(7, 4)] + b + [crop(1, 2, 9, 2)],
                  "HWC", _imgs([(6, 9, 3)], dtype, 90)))
    # pointwise: each threshold kind at the threshold, normalize per channel
    for kind in cases.THRESHOLD_KINDS:
        g.append(([threshold(127.0, kind, 200.0)], "HWC",
                  _imgs([(3, 5, 3)], dtype, 100)))
    g.append(([resize(4, 4), normalize([0.485, 0.456, 0.406],
                                       [0.229, 0.224, 0.225])], "CHW",
              _imgs([(9, 9, 3)], dtype, 101)))
    g.append(([color("gray"), threshold(50.0, "tozero"),
               threshold(200.0, "trunc"), normalize([0.1], [2.0]),
               threshold(0.2, "binary", 300.0)], "HWC",
              _imgs([(5, 6, 3), (5, 6, 1)], dtype, 102)))
    return g


def _compare(groups, out_type):
    ref, ref_flat = cases.run_plans(groups, out_type, "cpu")
    got, got_flat = cases.run_plans(groups, out_type, "cuda")
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.array_equal(a, b), (k, a.shape)
    # the gaps between images keep the canary: nothing is written outside
    assert np.array_equal(got_flat, ref_flat)
    return got_flat


@requires_gpu
@pytest.mark.parametrize("out_type", ["uint8", "float32"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_every_case_alone(dtype, out_type):
    for grp in _groups(dtype):
        _compare([grp], out_type)


@requires_gpu
@pytest.mark.parametrize("out_type", ["uint8", "float32"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_257_mixed_images_in_one_launch_twice(dtype, out_type):
    groups = _groups(dtype)
    n = sum(len(g[2]) for g in groups)
    k = 0
    while n < 257:                       # fill up by repeating cases
        groups.append(groups[k])
        n += len(groups[k][2])
        k += 1
    assert n >= 257
    a = _compare(groups, out_type)
    b = _compare(groups, out_type)
    assert np.array_equal(a, b)


@requires_gpu
def test_uint8_clamp_fires_at_both_ends():
    imgs = _imgs([(4, 70, 3)], np.float32, 5)
    assert imgs[0].min() < 0 and imgs[0].max() > 255
    out = _compare([([], "HWC", imgs)], "uint8")
    assert out.min() == 0 and out.max() == 255


@requires_gpu
def test_output_rows_that_are_not_dword_aligned():
    # 5 x 3 bytes per row: every row but the first starts off a dword
    _compare([([resize(6, 5)], "HWC", _imgs([(3, 3, 3), (7, 2, 3)],
                                            np.uint8, 6)),
              ([crop(0, 0, 3, 3)], "CHW", _imgs([(4, 4, 1)], np.uint8, 7))],
             "uint8")


@requires_gpu
def test_empty_batch_and_device_mismatch():
    got, flat = cases.run_plans([], "float32", "cuda")
    assert got == [] and flat.size == 0
    from mmlspark_amd.models.images import compile_image_plan
    plan = compile_image_plan([], [(2, 2, 1)], np.uint8, "uint8", "HWC")
    with pytest.raises(ValueError, match="share a device"):
        backend.image_preprocess(
            torch.zeros(4, dtype=torch.uint8), plan.idesc, plan.fdesc,
            plan.work_off, torch.zeros(4, dtype=torch.uint8, device="cuda"))


@requires_gpu
def test_work_items_agree_with_the_extension():
    from mmlspark_amd.ops import _hip_ops
    for h, w in [(1, 1), (8, 64), (9, 65), (224, 224), (32768, 32768)]:
        assert _hip_ops.image_work_items(h, w) == backend.image_work_items(h, w)


# ------------------------------------------------------------ public surface
@requires_gpu
def test_image_transformer_fused_mixed_column(monkeypatch):
    from mmlspark_amd.models import images
    from mmlspark_amd.utils import devices
    rng = np.random.default_rng(8)
    df = pd.DataFrame({"image": [
        cases.rand_image(rng, h, w, 3) for h, w in
        [(30, 40), (17, 9), (40, 30), (30, 40), (8, 64), (65, 66)]]})
    t = images.ImageTransformer(fused=True).crop(1, 2, 60, 60).flip(1) \
        .resize(24, 20).colorFormat("bgr2rgb")
    got = list(t.transform(df)["out_image"])
    unfused = images.ImageTransformer(stages=t.get("stages")).transform(df)
    with monkeypatch.context() as m:
        m.setattr(devices, "default_device",
                  lambda pref="auto": torch.device("cpu"))
        cpu = list(t.transform(df)["out_image"])
    for g, c, u in zip(got, cpu, unfused["out_image"]):
        assert g.dtype == np.uint8 and g.shape == (24, 20, 3)
        assert np.array_equal(g, c)
        assert np.abs(g.astype(np.int16) - u.astype(np.int16)).max() <= 1
    r = images.ResizeImageTransformer(height=7, width=70, fused=True)
    got = list(r.transform(df)["image"])
    with monkeypatch.context() as m:
        m.setattr(devices, "default_device",
                  lambda pref="auto": torch.device("cpu"))
        cpu = list(r.transform(df)["image"])
    for g, c in zip(got, cpu):
        assert g.dtype == np.uint8 and np.array_equal(g, c)


def _featurizers():
    from mmlspark_amd.models.image_featurizer import ImageFeaturizer
    plain = ImageFeaturizer(modelName="ResNet18", imageSize=64, device="cuda",
                            decodeOnDevice=True)
    fused = ImageFeaturizer(modelName="ResNet18", imageSize=64, device="cuda",
                            decodeOnDevice=True, fusedPreprocess=True
                            ).setModel(plain.module)
    return plain, fused


@requires_gpu
def test_featurizer_fused_uniform_batch_equals_unfused():
    pytest.importorskip("mmlspark_amd.io_http._jpeg_native")
    plain, fused = _featurizers()
    blobs = np.array([jpeg_codec.encode_jpeg(jcases.image(64, 64, s), 90)
                      for s in range(6)], dtype=object)
    got = fused._coerce(blobs)
    assert got.is_cuda and tuple(got.shape) == (6, 3, 64, 64)
    assert torch.equal(got, plain._coerce(blobs))


@requires_gpu
def test_featurizer_fused_mixed_sizes_and_gray():
    pytest.importorskip("mmlspark_amd.io_http._jpeg_native")
    from mmlspark_amd.io_http.jpeg_device import decode_jpeg_batch
    _, fused = _featurizers()
    blobs = [jpeg_codec.encode_jpeg(jcases.image(n, n, s), 90)
             for s, n in enumerate((48, 64, 48, 64))]
    blobs.append(jpeg_codec.encode_jpeg(jcases.image(40, 56, 9)[:, :, 0], 90))
    got = fused._coerce(np.array(blobs, dtype=object))
    assert got.is_cuda and tuple(got.shape) == (5, 3, 64, 64)
    pixels = [t.cpu().numpy() for t in decode_jpeg_batch(blobs, "cuda")]
    assert pixels[4].ndim == 2
    pixels = [p if p.ndim == 3 else p[:, :, None] for p in pixels]
    st = [resize(64, 64), color("_replicate3"), normalize([0.0], [1.0])]
    ref, _ = cases.run_plans([(st, "CHW", [p]) for p in pixels], "float32")
    assert np.array_equal(got.cpu().numpy(), np.stack(ref))
    F = np.stack(fused.transform(pd.DataFrame({"image": blobs}))
                 ["features"].to_numpy())
    assert F.shape[0] == 5 and F.shape[1] >= 128
    assert np.isfinite(F).all()
