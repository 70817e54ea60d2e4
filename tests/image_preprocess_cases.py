"""Shared cases for the image_preprocess tests: seeded images, stage lists,
a batch runner over ops.backend.image_preprocess, and an independent float64
oracle of the bilinear resize whose source coordinates are exact rationals.

The oracle shares no code with cpu_ref: it walks each axis with `Fraction`
(src = n_in/n_out * (d + 1/2) - 1/2, clamped at 0), turns the two tap
weights into float64 once per index and blends in float64, so its error is
a few float64 roundings — nothing against the float32 bound under test."""
from fractions import Fraction

import numpy as np
import torch

THRESHOLD_KINDS = ("binary", "binary_inv", "trunc", "tozero", "tozero_inv")


def rand_image(rng, H, W, C, dtype=np.uint8):
    """(H, W, C) image; float32 images carry fractions and values beyond
    0..255 so the uint8 clamp is exercised at both ends."""
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 256, size=(H, W, C), dtype=np.uint8)
    return rng.uniform(-40.0, 300.0, size=(H, W, C)).astype(np.float32)


def apply_chain(img, stages, as_uint8):
    """Today's per-image path: _to_tensor, _apply_stage per stage, _to_array."""
    from mmlspark_amd.models.images import _apply_stage, _to_array, _to_tensor
    t = _to_tensor(img)
    for st in stages:
        t = _apply_stage(t, st)
    return _to_array(t, as_uint8)


def _oracle_axis(n_in, n_out):
    i0s, i1s, l1s = [], [], []
    for d in range(n_out):
        src = Fraction(n_in, n_out) * (d + Fraction(1, 2)) - Fraction(1, 2)
        src = max(src, Fraction(0))
        i0 = min(src.numerator // src.denominator, n_in - 1)
        i0s.append(i0)
        i1s.append(min(i0 + 1, n_in - 1))
        l1s.append(float(src - i0))
    return np.array(i0s), np.array(i1s), np.array(l1s, dtype=np.float64)


def oracle_resize(img, Hr, Wr):
    """float64 bilinear resize (align_corners=False, no antialias) of an
    (H, W, C) image with exact rational source coordinates."""
    a = np.asarray(img, dtype=np.float64)
    y0, y1, ly = _oracle_axis(a.shape[0], Hr)
    x0, x1, lx = _oracle_axis(a.shape[1], Wr)
    lx, ly = lx[None, :, None], ly[:, None, None]
    top = (1.0 - lx) * a[y0][:, x0] + lx * a[y0][:, x1]
    bot = (1.0 - lx) * a[y1][:, x0] + lx * a[y1][:, x1]
    return (1.0 - ly) * top + ly * bot


def run_plans(groups, out_type, device="cpu"):
    """groups: [(stages, layout, [images...]), ...], all images of one
    dtype.  Compiles one plan per group, joins them into ONE
    image_preprocess call on `device` and returns the results, a numpy array
    per image in group order, together with the flat output buffer."""
    from mmlspark_amd.models.images import compile_image_plan
    from mmlspark_amd.ops import backend
    idesc, fdesc, work, srcs, spans = [], [], [0], [], []
    src_at = out_at = 0
    dtype = np.uint8
    for stages, layout, imgs in groups:
        dtype = imgs[0].dtype
        plan = compile_image_plan(
            stages, [im.shape for im in imgs], dtype, out_type, layout)
        assert plan is not None, stages
        d = plan.idesc.clone()
        d[:, 0] += src_at
        d[:, 18] += out_at
        idesc.append(d)
        fdesc.append(plan.fdesc)
        w = plan.work_off[1:] + work[-1]
        work.extend(w.tolist())
        srcs.extend(im.reshape(-1) for im in imgs)
        spans.extend((out_at + o, s) for o, s in
                     zip(plan.out_off.tolist(), plan.out_shapes))
        src_at += plan.src_numel
        out_at += (plan.out_numel + 3) // 4 * 4
    src_t = torch.uint8 if dtype == np.uint8 else torch.float32
    out_t = torch.uint8 if out_type == "uint8" else torch.float32
    src = torch.from_numpy(np.concatenate(srcs)) if srcs \
        else torch.empty(0, dtype=src_t)
    # a canary fill: bytes the plan does not own must come back untouched
    out = torch.full((out_at,), 7, dtype=out_t, device=device)
    from mmlspark_amd.ops.cpu_ref import IMG_DESC_F, IMG_DESC_I
    backend.image_preprocess(
        src.to(device),
        torch.cat(idesc) if idesc else torch.empty(0, IMG_DESC_I,
                                                   dtype=torch.int64),
        torch.cat(fdesc) if fdesc else torch.empty(0, IMG_DESC_F),
        torch.tensor(work, dtype=torch.int64), out)
    flat = out.cpu().numpy()
    res = [flat[o:o + int(np.prod(s))].reshape(s) for o, s in spans]
    return res, flat


# --------------------------------------------------------------- stage lists
def crop(x, y, h, w):
    return {"op": "crop", "x": x, "y": y, "height": h, "width": w}


def flip(code):
    return {"op": "flip", "flipCode": code}


def resize(h, w):
    return {"op": "resize", "height": h, "width": w}


def color(fmt):
    return {"op": "colorFormat", "format": fmt}


def threshold(thr, kind, mx=255.0):
    return {"op": "threshold", "threshold": thr, "maxVal": mx,
            "thresholdType": kind}


def normalize(mean, std):
    return {"op": "normalize", "mean": mean, "std": std}


def no_resize_cases():
    """(name, stages, [(H, W, C), ...]) — plans without a resize, which
    must reproduce the _apply_stage chain bit for bit."""
    cases = [("thr_" + k, [threshold(127.0, k, 200.0)], [(5, 7, 3), (4, 4, 1)])
             for k in THRESHOLD_KINDS]
    cases += [
        ("gray", [color("gray")], [(6, 5, 1), (6, 5, 3), (3, 9, 4)]),
        ("bgr2rgb", [color("bgr2rgb")], [(6, 5, 1), (6, 5, 3), (3, 9, 4)]),
        ("bgr2rgb_gray", [color("bgr2rgb"), color("gray")],
         [(6, 5, 3), (3, 9, 4), (2, 2, 1)]),
        ("norm_scalar", [normalize([0.45], [0.225])], [(5, 7, 3), (4, 4, 1)]),
        ("norm_channel", [normalize([0.485, 0.456, 0.406],
                                    [0.229, 0.224, 0.225])], [(5, 7, 3)]),
        ("gray_thr_norm", [color("gray"), threshold(100.0, "tozero"),
                           normalize([0.5], [0.25])], [(9, 8, 3), (9, 8, 1)]),
        ("crop_clipped", [crop(3, 2, 10, 10)], [(5, 7, 3), (12, 13, 1),
                                                (3, 4, 4)]),
        ("crop_crop", [crop(1, 1, 6, 6), crop(2, 0, 3, 9)], [(8, 8, 3),
                                                             (5, 4, 3)]),
        ("flip_h", [flip(1)], [(4, 6, 3)]),
        ("flip_v", [flip(0)], [(4, 6, 3)]),
        ("flip_both", [flip(-1)], [(4, 6, 3), (1, 5, 1)]),
        ("flip_crop_flip", [flip(1), crop(1, 2, 4, 3), flip(0),
                            crop(0, 1, 9, 9), flip(-1)],
         [(9, 8, 3), (7, 5, 1)]),
        ("four_ops", [threshold(50.0, "tozero"), threshold(200.0, "trunc"),
                      normalize([0.1], [2.0]), threshold(0.2, "binary", 1.0)],
         [(5, 5, 3)]),
    ]
    return cases
