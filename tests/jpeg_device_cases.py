"""Chosen streams for the device JPEG decode, shared by the CPU and GPU test
files: the smallest geometries at which descriptor indexing, cropping or
chroma replication can go wrong, and crafted streams that the coefficient
export and the parser must reject."""
import functools
import struct

import numpy as np

from mmlspark_amd.io_http import jpeg_codec
from mmlspark_amd.io_http.jpeg_codec import (HT_AC_L, HT_DC_L, _BitWriter,
                                             _build_codes)

from .test_jpeg_native import (_test_image, encode_baseline_sub,
                               encode_progressive)


def image(w, h, seed):
    """RGB test image, w pixels across and h down."""
    return _test_image(h=h, w=w, seed=seed)


@functools.lru_cache(maxsize=None)
def small_streams():
    """name -> stream.  Sizes are width x height."""
    checker = (np.indices((16, 16)).sum(0) % 2 * 255).astype(np.uint8)
    return {
        # one block; a crop inside padded blocks
        "gray_8x8": jpeg_codec.encode_jpeg(image(8, 8, 1)[:, :, 0], 90),
        "gray_9x7": jpeg_codec.encode_jpeg(image(9, 7, 2)[:, :, 1], 90),
        "444_8x8": jpeg_codec.encode_jpeg(image(8, 8, 3), 90),
        "444_17x9": jpeg_codec.encode_jpeg(image(17, 9, 4), 90),
        # one MCU; four MCUs cropped
        "420_16x16": encode_baseline_sub(image(16, 16, 5), 90, (2, 2)),
        "420_17x17": encode_baseline_sub(image(17, 17, 6), 90, (2, 2)),
        "422h_33x9": encode_baseline_sub(image(33, 9, 7), 90, (2, 1)),
        "422v_9x33": encode_baseline_sub(image(9, 33, 8), 90, (1, 2)),
        # 0/255 checkerboard at q=10: both clamps fire
        "checker_16x16": jpeg_codec.encode_jpeg(
            np.stack([checker] * 3, -1), 10),
        "prog_24x40": encode_progressive(image(24, 40, 9), 90),
        "base_24x40": jpeg_codec.encode_jpeg(image(24, 40, 9), 90),
    }


@functools.lru_cache(maxsize=None)
def large_streams():
    """120 rows x 200 columns at three qualities: 216,000 samples."""
    return tuple(jpeg_codec.encode_jpeg(_test_image(seed=q), q)
                 for q in (50, 90, 95))


def mixed_corpus():
    """Every small stream plus the large ones — mixed geometry for one
    call."""
    return list(small_streams().values()) + list(large_streams())


# ------------------------------------------------------- comparison rule
class Pool:
    """The comparison rule against the host decoder: equal shape and
    max |diff| <= 1 per image; pooled over a corpus of at least 200k
    samples, at most 0.1 % of samples differ at all."""

    def __init__(self):
        self.samples = 0
        self.differing = 0

    def add(self, got, ref):
        got, ref = np.asarray(got), np.asarray(ref)
        assert got.shape == ref.shape, (got.shape, ref.shape)
        assert got.dtype == np.uint8
        d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        assert d.max() <= 1, int(d.max())
        self.samples += d.size
        self.differing += int((d != 0).sum())

    def check(self):
        assert self.samples >= 200_000, self.samples
        print("differing samples: %d of %d" % (self.differing, self.samples))
        assert self.differing <= 0.001 * self.samples, \
            (self.differing, self.samples)


# -------------------------------------------------------- crafted streams
def _sof_at(b):
    p = b.index(b"\xff\xc0")
    return p + 4  # first byte of the SOF payload (sample precision)


def _patched(stream, offset_in_sof, value):
    b = bytearray(stream)
    b[_sof_at(b) + offset_in_sof] = value
    return bytes(b)


def _base_color():
    return encode_baseline_sub(image(16, 16, 5), 90, (2, 2))


def two_component_frame():
    b = bytearray(_base_color())
    s = _sof_at(b)
    b[s + 5] = 2                                  # component count
    del b[s + 6 + 6:s + 6 + 9]                    # drop the third component
    b[s - 2:s] = struct.pack(">H", 2 + 6 + 6)     # segment length
    return bytes(b)


def dc_overflow_stream():
    """Gray 8 x 200: every block's DC difference is +2047, so the DC
    coefficient passes 32767 at the 17th block."""
    enc = jpeg_codec.encode_jpeg(np.zeros((200, 8), np.uint8), 90)
    p = enc.index(b"\xff\xda")
    head = enc[:p + 2 + struct.unpack(">H", enc[p + 2:p + 4])[0]]
    dc, ac = _build_codes(*HT_DC_L), _build_codes(*HT_AC_L)
    bw = _BitWriter()
    for _ in range(25):
        bw.write(*dc[11])
        bw.write(2047, 11)
        bw.write(*ac[0x00])
    bw.flush()
    return head + bytes(bw.out) + b"\xff\xd9"


def invalid_for_export():
    """name -> stream that decode_jpeg_coefficients must reject (one per
    line of the export's validation list)."""
    base = _base_color()
    # SOF payload: P, H(2), W(2), Nc, then (id, hv, tq) per component
    return {
        "precision_12": _patched(base, 0, 12),
        "two_components": two_component_frame(),
        "h_zero": _patched(base, 7, 0x02),
        "h_five": _patched(base, 7, 0x52),
        "v_five": _patched(base, 7, 0x25),
        "hmax_not_multiple": _patched(_patched(base, 7, 0x31), 10, 0x21),
        "vmax_not_multiple": _patched(_patched(base, 7, 0x13), 10, 0x12),
        "luma_subsampled": _patched(_patched(base, 7, 0x11), 10, 0x21),
        "tq_4": _patched(base, 8, 4),
        "width_zero": _patched(_patched(base, 3, 0), 4, 0),
        "height_zero": _patched(_patched(base, 1, 0), 2, 0),
        # 8193 x 8193 > 2^26
        "too_many_pixels": _patched(_patched(_patched(_patched(
            base, 1, 0x20), 2, 0x01), 3, 0x20), 4, 0x01),
        "coefficient_over_int16": dc_overflow_stream(),
    }


def _seg(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) \
        + payload


def malformed_for_parser():
    """name -> stream the shared parser must reject without touching memory
    it does not own."""
    base = _base_color()
    out = {}
    # DHT whose bit counts sum to 510 symbols for a 256-entry table
    big = _seg(0xC4, bytes([0x00]) + bytes([255, 255] + [0] * 14)
               + bytes(510))
    out["dht_oversized"] = base[:2] + big + base[2:]
    for tid in range(4, 16):
        out["dqt_id_%d" % tid] = base[:2] + _seg(
            0xDB, bytes([tid]) + bytes([1] * 64)) + base[2:]
        out["dht_id_%d" % tid] = base[:2] + _seg(
            0xC4, bytes([tid]) + bytes([1] + [0] * 15) + bytes([0])) + base[2:]
        out["sof_tq_%d" % tid] = _patched(base, 8, tid)
        b = bytearray(base)
        p = b.index(b"\xff\xda")
        b[p + 6] = (tid << 4) | tid               # first component's Td/Ta
        out["sos_id_%d" % tid] = bytes(b)
    out["two_components"] = two_component_frame()
    out["h_zero"] = _patched(base, 7, 0x02)
    out["chroma_h_exceeds_luma"] = _patched(_patched(base, 7, 0x11), 10, 0x21)
    b = bytearray(base)
    p = b.index(b"\xff\xdb")
    b[p + 2:p + 4] = b"\xff\xff"                  # length runs past the end
    out["segment_past_end"] = bytes(b)
    b = bytearray(base)
    p = b.index(b"\xff\xda")
    out["sos_ss_gt_se"] = bytes(b[:p + 11] + bytes([5, 3, 0]) + b[p + 14:])
    out["sos_se_64"] = bytes(b[:p + 11] + bytes([0, 64, 0]) + b[p + 14:])
    out["sos_al_14"] = bytes(b[:p + 11] + bytes([0, 63, 14]) + b[p + 14:])
    out["seglen_1"] = base[:2] + b"\xff\xe0\x00\x01" + base[2:]
    return out


def fuzz_mutations():
    """The 150 seeded mutations of test_malformed_streams_never_crash."""
    img = (np.random.default_rng(0).integers(0, 255, (48, 48, 3))
           ).astype(np.uint8)
    enc = jpeg_codec.encode_jpeg(img, quality=80)
    rng = np.random.default_rng(1)
    out = []
    for trial in range(150):
        b = bytearray(enc)
        mode = trial % 3
        if mode == 0:
            b = b[:rng.integers(2, len(b))]
        elif mode == 1:
            for _ in range(rng.integers(1, 8)):
                b[rng.integers(0, len(b))] = rng.integers(0, 256)
        else:
            b = bytes([0xFF, 0xD8]) + bytes(
                rng.integers(0, 256, rng.integers(10, 300)).astype(np.uint8))
        out.append(bytes(b))
    return out
