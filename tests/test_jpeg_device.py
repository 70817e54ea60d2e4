"""Device JPEG decode, the parts that need no GPU: the coefficient export,
batch packing and descriptor check (through the torch reference), rejection
of everything the device would index with, and a sanitizer run of the shared
parser on malformed streams."""
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

from mmlspark_amd.io_http import jpeg_codec
from mmlspark_amd.ops import backend, cpu_ref

from . import jpeg_device_cases as cases

_jpeg_native = pytest.importorskip("mmlspark_amd.io_http._jpeg_native")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _single_image_descriptors(W, H, comps, out_off=0):
    nc = len(comps)
    img_desc = torch.tensor([[W, H, nc, out_off]], dtype=torch.int64)
    comp_desc = torch.zeros(1, 3, 4, dtype=torch.int64)
    for ci, (h, v, tq, _bw, _bh, off) in enumerate(comps):
        comp_desc[0, ci] = torch.tensor([h, v, tq, off])
    items = int(backend.jpeg_work_items(W, H, comps[0][0], comps[0][1]))
    work_off = torch.tensor([0, items], dtype=torch.int64)
    return img_desc, comp_desc, work_off


def _reconstruct_one(stream):
    coef, qt, W, H, comps = _jpeg_native.decode_jpeg_coefficients(stream)
    nc = len(comps)
    out = torch.zeros(H * W * nc, dtype=torch.uint8)
    cpu_ref.jpeg_reconstruct(coef, qt.unsqueeze(0),
                             *_single_image_descriptors(W, H, comps), out)
    return out.view((H, W, 3) if nc == 3 else (H, W)).numpy()


def test_export_layout():
    """int16 (blocks, 64) zigzag planes, component by component; uint16
    tables; geometry of a 4:2:0 17x17 frame."""
    coef, qt, W, H, comps = _jpeg_native.decode_jpeg_coefficients(
        cases.small_streams()["420_17x17"])
    assert (W, H) == (17, 17)
    assert comps == [(2, 2, 0, 4, 4, 0), (1, 1, 1, 2, 2, 16),
                     (1, 1, 1, 2, 2, 20)]
    assert coef.dtype == torch.int16 and tuple(coef.shape) == (24, 64)
    assert qt.dtype == torch.uint16 and tuple(qt.shape) == (4, 64)
    ql, qc = jpeg_codec._quality_tables(90)
    zz = np.asarray(jpeg_codec.ZIGZAG)
    np.testing.assert_array_equal(qt.to(torch.int32).numpy()[0],
                                  ql.reshape(-1)[zz])
    np.testing.assert_array_equal(qt.to(torch.int32).numpy()[1],
                                  qc.reshape(-1)[zz])


def test_export_reconstructs_like_the_host_decoder():
    pool = cases.Pool()
    for s in cases.mixed_corpus():
        pool.add(_reconstruct_one(s), _jpeg_native.decode_jpeg(s).numpy())
    pool.check()


def test_batch_on_cpu_matches_the_host_decoder():
    from mmlspark_amd.io_http.jpeg_device import decode_jpeg_batch
    corpus = cases.mixed_corpus()
    outs = decode_jpeg_batch(corpus, "cpu")
    assert len(outs) == len(corpus)
    pool = cases.Pool()
    for s, o in zip(corpus, outs):
        assert o.dtype == torch.uint8 and o.device.type == "cpu"
        pool.add(o.numpy(), _jpeg_native.decode_jpeg(s).numpy())
    pool.check()
    # views of one allocation
    base = outs[0].untyped_storage().data_ptr()
    assert all(o.untyped_storage().data_ptr() == base for o in outs)


def test_batch_thread_count_and_empty():
    from mmlspark_amd.io_http.jpeg_device import decode_jpeg_batch
    assert decode_jpeg_batch([], "cpu") == []
    corpus = list(cases.small_streams().values())
    a = decode_jpeg_batch(corpus, "cpu", num_threads=1)
    b = decode_jpeg_batch(corpus, "cpu", num_threads=64)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_progressive_equals_baseline_on_cpu():
    from mmlspark_amd.io_http.jpeg_device import decode_jpeg_batch
    s = cases.small_streams()
    p, b = decode_jpeg_batch([s["prog_24x40"], s["base_24x40"]], "cpu")
    assert tuple(p.shape) == (40, 24, 3)
    assert torch.equal(p, b)


# ------------------------------------------------------------ bad input
def _valid_descriptors():
    coef, qt, W, H, comps = _jpeg_native.decode_jpeg_coefficients(
        cases.small_streams()["420_17x17"])
    return (coef.shape[0], qt.unsqueeze(0),
            *_single_image_descriptors(W, H, comps), H * W * 3)


def test_descriptor_check_accepts_a_valid_batch():
    backend.check_jpeg_descriptors(*_valid_descriptors())


def test_descriptor_check_rejects_block_offset_one_past_the_end():
    n_blocks, qt, img, comp, work, nbytes = _valid_descriptors()
    comp[0, 2, 3] += 1
    with pytest.raises(ValueError, match="coefficient buffer"):
        backend.check_jpeg_descriptors(n_blocks, qt, img, comp, work, nbytes)
    # and the dispatching op refuses before it reconstructs anything
    coef = torch.zeros(n_blocks, 64, dtype=torch.int16)
    out = torch.zeros(nbytes, dtype=torch.uint8)
    with pytest.raises(ValueError):
        backend.jpeg_reconstruct(coef, qt, img, comp, work, out)
    assert not out.any()


def test_descriptor_check_rejects_output_one_byte_short():
    n_blocks, qt, img, comp, work, nbytes = _valid_descriptors()
    with pytest.raises(ValueError, match="output buffer"):
        backend.check_jpeg_descriptors(n_blocks, qt, img, comp, work,
                                       nbytes - 1)
    img[0, 3] = 1
    with pytest.raises(ValueError, match="output buffer"):
        backend.check_jpeg_descriptors(n_blocks, qt, img, comp, work, nbytes)


def test_descriptor_check_rejects_bad_tables_and_prefix_sums():
    n_blocks, qt, img, comp, work, nbytes = _valid_descriptors()
    bad = comp.clone()
    bad[0, 1, 2] = 4
    with pytest.raises(ValueError, match="table id"):
        backend.check_jpeg_descriptors(n_blocks, qt, img, bad, work, nbytes)
    for w in ([0, 3], [1, 5], [4, 0]):
        with pytest.raises(ValueError, match="prefix sum"):
            backend.check_jpeg_descriptors(
                n_blocks, qt, img, comp, torch.tensor(w, dtype=torch.int64),
                nbytes)
    bad = comp.clone()
    bad[0, 1, 0] = 3  # 2 % 3: chroma factor does not divide luma's
    with pytest.raises(ValueError):
        backend.check_jpeg_descriptors(n_blocks, qt, img, bad, work, nbytes)


@pytest.mark.parametrize("name", sorted(cases.invalid_for_export()))
def test_export_rejects(name):
    from mmlspark_amd.io_http.jpeg_device import decode_jpeg_batch
    stream = cases.invalid_for_export()[name]
    with pytest.raises(RuntimeError):
        _jpeg_native.decode_jpeg_coefficients(stream)
    good = cases.small_streams()["444_8x8"]
    with pytest.raises(ValueError):
        decode_jpeg_batch([good, stream], "cpu")


def test_parser_rejects_malformed_streams_in_both_entry_points():
    for name, stream in cases.malformed_for_parser().items():
        for fn in (_jpeg_native.decode_jpeg,
                   _jpeg_native.decode_jpeg_coefficients):
            with pytest.raises(RuntimeError):
                fn(stream)
                pytest.fail("accepted " + name)


def test_parser_is_clean_under_sanitizers(tmp_path):
    """tools/jpeg_parse_fuzz.cpp, built with ASan + UBSan, runs parse +
    export over the malformed corpus: every stream decodes or throws, and
    the sanitizers see no invalid access."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ to build the sanitizer harness")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run([cxx] + san + [str(probe), "-o",
                                           str(tmp_path / "probe")],
                            capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("compiler cannot link the sanitizer runtime: "
                    + linked.stderr[-300:])
    exe = tmp_path / "jpeg_parse_fuzz"
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g"] + san
        + ["-I", os.path.join(ROOT, "mmlspark_amd", "io_http"),
           os.path.join(ROOT, "tools", "jpeg_parse_fuzz.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    corpus = dict(cases.malformed_for_parser())
    corpus.update(cases.invalid_for_export())
    corpus.update({"fuzz_%03d" % i: s
                   for i, s in enumerate(cases.fuzz_mutations())})
    corpus["valid_420"] = cases.small_streams()["420_17x17"]
    corpus["valid_prog"] = cases.small_streams()["prog_24x40"]
    paths = []
    for name, stream in corpus.items():
        p = tmp_path / (name + ".jpg")
        p.write_bytes(stream)
        paths.append(str(p))
    run = subprocess.run([str(exe)] + paths, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert "%d streams" % len(paths) in run.stdout, run.stdout


# ----------------------------------------------------------- featurizer
def test_featurizer_decode_on_device_is_the_host_path_on_cpu():
    from mmlspark_amd.models.image_featurizer import ImageFeaturizer
    blobs = [jpeg_codec.encode_jpeg(cases.image(64, 64, s), 90)
             for s in (1, 2, 3)]
    df = pd.DataFrame({"image": blobs})
    torch.manual_seed(0)
    ref = ImageFeaturizer(modelName="ResNet18", imageSize=64, device="cpu")
    assert ref.get("decodeOnDevice") is False
    dev = ImageFeaturizer(modelName="ResNet18", imageSize=64, device="cpu",
                          decodeOnDevice=True).setModel(ref.module)
    assert torch.equal(dev._coerce(df["image"].to_numpy()),
                       ref._coerce(df["image"].to_numpy()))
    a = np.stack(ref.transform(df)["features"].to_numpy())
    b = np.stack(dev.transform(df)["features"].to_numpy())
    np.testing.assert_array_equal(a, b)
