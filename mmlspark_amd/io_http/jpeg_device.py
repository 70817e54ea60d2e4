"""Decode a batch of JPEG byte strings straight into device tensors.

The split follows the data: Huffman decoding is serial per stream and stays
on CPU threads (``_jpeg_native.decode_jpeg_coefficients``, GIL released);
dequantisation, IDCT, chroma upsampling, colour conversion and the crop are
data-parallel and run in one launch of ``jpeg_reconstruct_k``
(ops/hip/image_kernels.hip).  The batch crosses to the device once, as int16
coefficients (~2 bytes per sample) instead of 12-byte-per-pixel floats.

The device arithmetic is the host decoder's, operation for operation, so the
pixels are the ones ``jpeg_codec.decode_jpeg`` returns.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import List, Sequence

import torch

from ..ops import backend

_MAX_THREADS = 16


def _align(n: int, a: int) -> int:
    return (n + a - 1) // a * a


def _export(blob):
    from . import _jpeg_native
    return _jpeg_native.decode_jpeg_coefficients(bytes(blob))


def decode_jpeg_batch(blobs: Sequence[bytes], device,
                      num_threads: int = 16) -> List[torch.Tensor]:
    """JPEG byte strings -> uint8 tensors on ``device``, ``H×W×3`` (colour)
    or ``H×W`` (gray), in input order; all are views of one allocation.

    ``device="cpu"`` runs the same export, packing and descriptor check and
    reconstructs with the torch reference.  Malformed or unsupported streams
    raise ``ValueError`` (like ``jpeg_codec.decode_jpeg``)."""
    out, spans = decode_jpeg_batch_flat(blobs, device, num_threads)
    res = []
    for off, shape in spans:
        numel = shape[0] * shape[1] * (3 if len(shape) == 3 else 1)
        res.append(out[off:off + numel].view(shape))
    return res


def decode_jpeg_batch_flat(blobs: Sequence[bytes], device,
                           num_threads: int = 16):
    """The allocation behind ``decode_jpeg_batch``: (flat uint8 buffer on
    ``device``, [(offset, shape), ...]) with image i's pixels, HWC, at its
    dword-aligned offset — what ``ops.backend.image_preprocess`` reads
    without a copy."""
    device = torch.device(device)
    n = len(blobs)
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=device), []
    workers = max(1, min(int(num_threads), _MAX_THREADS, n))
    try:
        if workers == 1:
            parts = [_export(b) for b in blobs]
        else:
            with ThreadPoolExecutor(max_workers=workers) as ex:
                parts = list(ex.map(_export, blobs))
    except RuntimeError as e:  # same error contract as jpeg_codec.decode_jpeg
        raise ValueError(str(e)) from e

    # ---- descriptors (layout in ops/hip/image_kernels.hip)
    img_rows, comp_rows, work, spans = [], [], [0], []
    block_at = out_at = 0
    for c, _q, W, H, comps in parts:
        nc = len(comps)
        img_rows.append((W, H, nc, out_at))
        rows = [(h, v, tq, block_at + off)
                for h, v, tq, _bw, _bh, off in comps]
        comp_rows.append(rows + [(0, 0, 0, 0)] * (3 - nc))
        block_at += c.shape[0]
        work.append(work[-1] + int(backend.jpeg_work_items(
            W, H, comps[0][0], comps[0][1])))
        spans.append((out_at, (H, W, 3) if nc == 3 else (H, W)))
        # images start dword-aligned so full rows can be stored as dwords
        out_at = _align(out_at + H * W * nc, 4)
    pin = device.type == "cuda"
    desc = torch.empty(n * 16 + n + 1, dtype=torch.int64, pin_memory=pin)
    img_desc = desc[:n * 4].view(n, 4)
    comp_desc = desc[n * 4:n * 16].view(n, 3, 4)
    work_off = desc[n * 16:]
    img_desc.copy_(torch.tensor(img_rows, dtype=torch.int64))
    comp_desc.copy_(torch.tensor(comp_rows, dtype=torch.int64))
    work_off.copy_(torch.tensor(work, dtype=torch.int64))

    # ---- one staging buffer: quantisation tables | coefficients
    total_blocks = block_at
    coef_at = n * 4 * 64 * 2
    stage = torch.empty(coef_at + total_blocks * 128, dtype=torch.uint8,
                        pin_memory=pin)

    def views(buf):
        return (buf[:coef_at].view(torch.uint16).view(n, 4, 64),
                buf[coef_at:].view(torch.int16).view(total_blocks, 64))

    qt, coef = views(stage)
    block_at = 0
    for i, (c, q, _W, _H, _comps) in enumerate(parts):
        qt[i] = q
        coef[block_at:block_at + c.shape[0]] = c
        block_at += c.shape[0]

    out = torch.empty(out_at, dtype=torch.uint8, device=device)
    if pin:
        qt, coef = views(stage.to(device, non_blocking=True))
    backend.jpeg_reconstruct(coef, qt, img_desc, comp_desc, work_off, out)
    return out, spans
