"""jpeg_reconstruct_k on MI355X: the smallest geometries at which the kernel
can go wrong, alone and mixed in one launch, against the host decoder."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from mmlspark_amd.io_http import jpeg_codec

from . import jpeg_device_cases as cases

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")

_jpeg_native = pytest.importorskip("mmlspark_amd.io_http._jpeg_native")

SMALL = ["gray_8x8", "gray_9x7", "444_8x8", "444_17x9", "420_16x16",
         "420_17x17", "422h_33x9", "422v_9x33", "checker_16x16"]


@functools.lru_cache(maxsize=None)
def _host(stream):
    """Host decode, computed once per stream and read-only."""
    a = _jpeg_native.decode_jpeg(stream).numpy()
    a.setflags(write=False)
    return a


def _decode(streams):
    from mmlspark_amd.io_http.jpeg_device import decode_jpeg_batch
    outs = decode_jpeg_batch(streams, "cuda")
    assert len(outs) == len(streams)
    for o in outs:
        assert o.is_cuda and o.dtype == torch.uint8
    return outs


def _assert_within_one(got, stream):
    ref = _host(stream)
    got = got.cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    assert d.max() <= 1, int(d.max())


@requires_gpu
@pytest.mark.parametrize("name", SMALL)
def test_single_small_image(name):
    stream = cases.small_streams()[name]
    (out,) = _decode([stream])
    _assert_within_one(out, stream)


@requires_gpu
def test_checkerboard_hits_both_clamps():
    stream = cases.small_streams()["checker_16x16"]
    ref = _host(stream)
    assert ref.min() == 0 and ref.max() == 255
    (out,) = _decode([stream])
    out = out.cpu().numpy()
    assert out.min() == 0 and out.max() == 255
    _assert_within_one(torch.from_numpy(out), stream)


@requires_gpu
def test_progressive_equals_baseline():
    s = cases.small_streams()
    p, b = _decode([s["prog_24x40"], s["base_24x40"]])
    assert tuple(p.shape) == (40, 24, 3)
    assert torch.equal(p, b)
    _assert_within_one(p, s["prog_24x40"])


@requires_gpu
def test_mixed_geometry_in_one_call():
    corpus = cases.mixed_corpus()
    outs = _decode(corpus)
    pool = cases.Pool()
    for s, o in zip(corpus, outs):
        pool.add(o.cpu().numpy(), _host(s))
    pool.check()
    # views of one allocation
    base = outs[0].untyped_storage().data_ptr()
    assert all(o.untyped_storage().data_ptr() == base for o in outs)


@requires_gpu
def test_257_images_in_one_call():
    s = cases.small_streams()
    four = [s["444_8x8"], s["gray_8x8"],
            jpeg_codec.encode_jpeg(cases.image(8, 8, 21), 50),
            jpeg_codec.encode_jpeg(cases.image(8, 8, 22), 95)]
    streams = [four[i % 4] for i in range(257)]
    outs = _decode(streams)
    for i in range(4):
        _assert_within_one(outs[i], four[i])
    for i, o in enumerate(outs):
        assert torch.equal(o, outs[i % 4]), i


@requires_gpu
def test_same_batch_twice_is_bit_identical():
    corpus = cases.mixed_corpus()
    a = _decode(corpus)
    b = _decode(corpus)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@requires_gpu
def test_empty_batch():
    from mmlspark_amd.io_http.jpeg_device import decode_jpeg_batch
    assert decode_jpeg_batch([], "cuda") == []


# ----------------------------------------------------------- featurizer
def _featurizers():
    from mmlspark_amd.models.image_featurizer import ImageFeaturizer
    host = ImageFeaturizer(modelName="ResNet18", imageSize=64, device="cuda")
    dev = ImageFeaturizer(modelName="ResNet18", imageSize=64, device="cuda",
                          decodeOnDevice=True).setModel(host.module)
    return host, dev


@requires_gpu
def test_featurizer_decode_on_device_uniform_batch():
    host, dev = _featurizers()
    blobs = np.array([jpeg_codec.encode_jpeg(cases.image(64, 64, s), 90)
                      for s in range(18)], dtype=object)
    got = dev._coerce(blobs)
    assert got.is_cuda and tuple(got.shape) == (18, 3, 64, 64)
    ref = host._coerce(blobs).to("cuda")
    diff = (got - ref).abs()
    off = diff != 0
    assert int(off.sum()) <= 0.001 * got.numel(), int(off.sum())
    # every differing element is one 8-bit step: |a/255 - b/255|, a-b = ±1
    steps = (got * 255.0).round() - (ref * 255.0).round()
    assert bool((steps[off].abs() == 1).all())
    assert bool((steps[~off] == 0).all())
    F = np.stack(dev.transform(pd.DataFrame({"image": list(blobs)}))
                 ["features"].to_numpy())
    assert F.shape[0] == 18 and F.shape[1] >= 128
    assert np.isfinite(F).all()


@requires_gpu
def test_featurizer_decode_on_device_mixed_sizes():
    _, dev = _featurizers()
    blobs = [jpeg_codec.encode_jpeg(cases.image(n, n, s), 90)
             for s, n in enumerate((48, 64, 48, 64, 64))]
    got = dev._coerce(np.array(blobs, dtype=object))
    assert got.is_cuda and tuple(got.shape) == (5, 3, 64, 64)
    F = np.stack(dev.transform(pd.DataFrame({"image": blobs}))
                 ["features"].to_numpy())
    assert F.shape[0] == 5 and F.shape[1] >= 128
    assert np.isfinite(F).all()
