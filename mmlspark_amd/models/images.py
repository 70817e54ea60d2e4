"""ImageTransformer / ImageSetAugmenter — the opencv module re-expressed on
torch image ops (opencv/src/main/scala/.../ImageTransformer.scala:282:
ResizeImage:42, CropImage:75, ColorFormat:102, Flip:122, Blur:148,
Threshold:172, GaussianKernel:199; ImageSetAugmenter.scala:18).

Stages are a recorded op list applied per image; tensors run on whatever
device is default, so the same code drives MIOpen-backed GPU kernels on
MI355X (interpolate/conv2d) — no OpenCV JNI."""
from __future__ import annotations


import numpy as np
import pandas as pd
import torch

from ..core.param import Param, toBool, toList, toString, toInt
from ..core.pipeline import Transformer
from ..core.registry import register


def _to_tensor(img) -> torch.Tensor:
    a = np.asarray(img)
    t = torch.from_numpy(np.ascontiguousarray(a)).float()
    if t.ndim == 2:
        t = t.unsqueeze(-1)
    return t  # (H, W, C) float


def _to_array(t: torch.Tensor, as_uint8: bool) -> np.ndarray:
    # clamp only on the uint8 path: float outputs (e.g. normalize, whose
    # values are signed) must pass through untouched
    if as_uint8:
        return t.clamp(0, 255).cpu().numpy().astype(np.uint8)
    return t.cpu().numpy()


def _apply_stage(t: torch.Tensor, stage: dict) -> torch.Tensor:
    op = stage["op"]
    if op == "resize":
        h, w = int(stage["height"]), int(stage["width"])
        x = t.permute(2, 0, 1).unsqueeze(0)
        x = torch.nn.functional.interpolate(x, size=(h, w), mode="bilinear",
                                            align_corners=False)
        return x.squeeze(0).permute(1, 2, 0)
    if op == "crop":
        x, y = int(stage["x"]), int(stage["y"])
        h, w = int(stage["height"]), int(stage["width"])
        return t[y:y + h, x:x + w]
    if op == "flip":
        code = int(stage.get("flipCode", 1))  # 1=horizontal, 0=vertical, -1=both
        if code >= 1:
            return torch.flip(t, dims=[1])
        if code == 0:
            return torch.flip(t, dims=[0])
        return torch.flip(t, dims=[0, 1])
    if op == "colorFormat":
        fmt = stage.get("format", "gray")
        if fmt in ("gray", "grayscale"):
            if t.shape[2] >= 3:
                gray = (0.299 * t[:, :, 2] + 0.587 * t[:, :, 1]
                        + 0.114 * t[:, :, 0])  # BGR convention like OpenCV
                return gray.unsqueeze(-1)
            return t
        if fmt == "bgr2rgb" and t.shape[2] >= 3:
            return t.flip(-1)
        return t
    if op == "blur":
        kh, kw = int(stage["height"]), int(stage["width"])
        kernel = torch.ones(1, 1, kh, kw, dtype=t.dtype) / (kh * kw)
        x = t.permute(2, 0, 1).unsqueeze(1)  # (C,1,H,W)
        x = torch.nn.functional.conv2d(x, kernel,
                                       padding=(kh // 2, kw // 2))
        return x.squeeze(1).permute(1, 2, 0)[:t.shape[0], :t.shape[1]]
    if op == "gaussianKernel":
        size = int(stage.get("apertureSize", 3))
        sigma = float(stage.get("sigma", 1.0))
        ax = torch.arange(size, dtype=t.dtype) - (size - 1) / 2.0
        g1 = torch.exp(-(ax ** 2) / (2 * sigma * sigma))
        k = (g1[:, None] * g1[None, :])
        k = k / k.sum()
        x = t.permute(2, 0, 1).unsqueeze(1)
        x = torch.nn.functional.conv2d(x, k.reshape(1, 1, size, size),
                                       padding=size // 2)
        return x.squeeze(1).permute(1, 2, 0)[:t.shape[0], :t.shape[1]]
    if op == "threshold":
        thr = float(stage["threshold"])
        mx = float(stage.get("maxVal", 255.0))
        kind = stage.get("thresholdType", "binary")
        if kind == "binary":
            return torch.where(t > thr, torch.full_like(t, mx),
                               torch.zeros_like(t))
        if kind == "binary_inv":
            return torch.where(t > thr, torch.zeros_like(t),
                               torch.full_like(t, mx))
        if kind == "trunc":
            return t.clamp_max(thr)
        if kind == "tozero":
            return torch.where(t > thr, t, torch.zeros_like(t))
        return torch.where(t > thr, torch.zeros_like(t), t)  # tozero_inv
    if op == "normalize":
        mean = torch.tensor(stage.get("mean", [0.0]), dtype=t.dtype)
        std = torch.tensor(stage.get("std", [1.0]), dtype=t.dtype)
        return (t / 255.0 - mean) / std
    raise ValueError(f"unknown image op {op!r}")


def _apply_stage_batched(t: torch.Tensor, stage: dict) -> torch.Tensor:
    """Batched (N, H, W, C) mirror of _apply_stage — uniform-shape batches
    run every op as ONE device launch instead of a per-image Python loop."""
    op = stage["op"]
    if op == "resize":
        h, w = int(stage["height"]), int(stage["width"])
        x = t.permute(0, 3, 1, 2)
        x = torch.nn.functional.interpolate(x, size=(h, w), mode="bilinear",
                                            align_corners=False)
        return x.permute(0, 2, 3, 1)
    if op == "crop":
        x, y = int(stage["x"]), int(stage["y"])
        h, w = int(stage["height"]), int(stage["width"])
        return t[:, y:y + h, x:x + w]
    if op == "flip":
        code = int(stage.get("flipCode", 1))
        if code >= 1:
            return torch.flip(t, dims=[2])
        if code == 0:
            return torch.flip(t, dims=[1])
        return torch.flip(t, dims=[1, 2])
    if op == "colorFormat":
        fmt = stage.get("format", "gray")
        if fmt in ("gray", "grayscale"):
            if t.shape[-1] >= 3:
                gray = (0.299 * t[..., 2] + 0.587 * t[..., 1]
                        + 0.114 * t[..., 0])
                return gray.unsqueeze(-1)
            return t
        if fmt == "bgr2rgb" and t.shape[-1] >= 3:
            return t.flip(-1)
        return t
    if op in ("blur", "gaussianKernel"):
        if op == "blur":
            kh, kw = int(stage["height"]), int(stage["width"])
            k = torch.ones(1, 1, kh, kw, dtype=t.dtype,
                           device=t.device) / (kh * kw)
        else:
            size = int(stage.get("apertureSize", 3))
            sigma = float(stage.get("sigma", 1.0))
            ax = (torch.arange(size, dtype=t.dtype, device=t.device)
                  - (size - 1) / 2.0)
            g1 = torch.exp(-(ax ** 2) / (2 * sigma * sigma))
            k = (g1[:, None] * g1[None, :])
            k = (k / k.sum()).reshape(1, 1, size, size)
            kh = kw = size
        N, H, W, C = t.shape
        x = t.permute(0, 3, 1, 2).reshape(N * C, 1, H, W)
        x = torch.nn.functional.conv2d(x, k, padding=(kh // 2, kw // 2))
        x = x[:, :, :H, :W].reshape(N, C, H, W).permute(0, 2, 3, 1)
        return x
    if op == "threshold":
        return _apply_stage(t, stage)   # purely elementwise
    if op == "normalize":
        mean = torch.tensor(stage.get("mean", [0.0]), dtype=t.dtype,
                            device=t.device)
        std = torch.tensor(stage.get("std", [1.0]), dtype=t.dtype,
                           device=t.device)
        return (t / 255.0 - mean) / std
    raise ValueError(f"unknown image op {op!r}")


# ------------------------------------------------------------ fused plans
# A stage list that fits the plan of ops.backend.image_preprocess (contract
# in docs/kernels.md) runs as ONE launch over a column of any mix of shapes:
# pre-window -> at most one bilinear resize -> post-window -> channel map ->
# at most four pointwise ops -> uint8 | float32, HWC | CHW.
_THRESHOLD_KINDS = {"binary": 0, "binary_inv": 1, "trunc": 2, "tozero": 3,
                    "tozero_inv": 4}
_OP_NORMALIZE = 5
_GRAY = 4                      # channel-map code of the gray combination
_MAX_DIM = 32768


class ImagePlan:
    """Descriptors of one batch for ops.backend.image_preprocess: the three
    descriptor tensors, where each source image starts in the flat source
    buffer and where (and in which shape) each result lies in the flat
    output buffer."""

    def __init__(self, idesc, fdesc, work_off, src_off, src_numel, out_off,
                 out_shapes, out_numel, src_dtype, out_dtype):
        self.idesc, self.fdesc, self.work_off = idesc, fdesc, work_off
        self.src_off, self.src_numel = src_off, src_numel
        self.out_off, self.out_shapes = out_off, out_shapes
        self.out_numel = out_numel
        self.src_dtype, self.out_dtype = src_dtype, out_dtype


def _crop_view(view, x, y, h, w) -> bool:
    """t[y:y+h, x:x+w] of a window [y0, x0, H, W, flip_y, flip_x] of its
    base image, clipped like Python slicing; False when nothing is left."""
    y0, x0, H, W, fy, fx = view
    if y >= H or x >= W:
        return False
    nh, nw = min(y + h, H) - y, min(x + w, W) - x
    view[0] = y0 + (H - y - nh if fy else y)
    view[1] = x0 + (W - x - nw if fx else x)
    view[2], view[3] = nh, nw
    return True


def _plan_one(stages, H, W, C):
    """One source shape through the stage list: (pre-window, resized size,
    post-window, channel map, gray operands, pointwise ops), windows as
    [y0, x0, H, W, flip_y, flip_x], or None when the stages do not fit the
    plan."""
    if not (1 <= H <= _MAX_DIM and 1 <= W <= _MAX_DIM and 1 <= C <= 4):
        return None
    pre = [0, 0, H, W, False, False]
    post = resized = None        # set by the resize
    chan = list(range(C))        # source channel, or _GRAY, per output
    gray_of = (0, 0, 0)
    ops = []                     # (kind, 8 floats)
    after_resize_only = False    # a gray / threshold / normalize was seen
    for st in stages:
        op = st["op"]
        view = pre if post is None else post
        if op == "crop":
            x, y = int(st["x"]), int(st["y"])
            h, w = int(st["height"]), int(st["width"])
            if x < 0 or y < 0 or h <= 0 or w <= 0 \
                    or not _crop_view(view, x, y, h, w):
                return None
        elif op == "flip":
            code = int(st.get("flipCode", 1))
            if code >= 1 or code < 0:
                view[5] = not view[5]
            if code <= 0:
                view[4] = not view[4]
        elif op == "resize":
            h, w = int(st["height"]), int(st["width"])
            if post is not None or after_resize_only \
                    or not (1 <= h <= _MAX_DIM and 1 <= w <= _MAX_DIM):
                return None
            resized, post = (h, w), [0, 0, h, w, False, False]
        elif op == "colorFormat":
            fmt = st.get("format", "gray")
            if fmt in ("gray", "grayscale") and len(chan) >= 3:
                if ops:
                    return None
                gray_of, chan = tuple(chan[:3]), [_GRAY]
                after_resize_only = True
            elif fmt == "bgr2rgb" and len(chan) >= 3:
                if ops:
                    return None
                chan = chan[::-1]
            elif fmt == "_replicate3" and len(chan) == 1:
                chan = chan * 3
        elif op == "threshold":
            if len(ops) == 4:
                return None
            kind = _THRESHOLD_KINDS.get(st.get("thresholdType", "binary"), 4)
            ops.append((kind, [float(st["threshold"]),
                               float(st.get("maxVal", 255.0))] + [0.0] * 6))
            after_resize_only = True
        elif op == "normalize":
            mean = [float(v) for v in np.atleast_1d(st.get("mean", [0.0]))]
            std = [float(v) for v in np.atleast_1d(st.get("std", [1.0]))]
            if len(ops) == 4 or len(mean) not in (1, len(chan)) \
                    or len(std) not in (1, len(chan)):
                return None
            mean = (mean * 4 if len(mean) == 1 else mean + [0.0] * 4)[:4]
            std = (std * 4 if len(std) == 1 else std + [1.0] * 4)[:4]
            ops.append((_OP_NORMALIZE, mean + std))
            after_resize_only = True
        else:                    # blur, gaussianKernel, anything unknown
            return None
    if post is None:
        resized, post = (pre[2], pre[3]), [0, 0, pre[2], pre[3], False, False]
    return pre, resized, post, chan, gray_of, ops


def compile_image_plan(stages, shapes, dtype, out_type, layout,
                       src_off=None):
    """Compile a stage list for a batch of source shapes [(H, W, C), ...]
    of one dtype (uint8 | float32) into the descriptors of
    ops.backend.image_preprocess, or None when the stages do not fit the
    plan (the caller then keeps the per-stage path).  `out_type` is
    "uint8" | "float32", `layout` "HWC" | "CHW".  Sources are packed back to
    back unless `src_off` gives each image's element offset; results start
    dword-aligned in one flat buffer.  The work is done once per distinct
    (H, W, C) and broadcast."""
    from ..ops import backend
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.uint8), np.dtype(np.float32)) \
            or layout not in ("HWC", "CHW") \
            or out_type not in ("uint8", "float32", "float"):
        return None
    out_u8 = out_type == "uint8"
    n = len(shapes)
    sh = np.asarray(shapes, dtype=np.int64).reshape(n, 3)
    uniq, inv = np.unique(sh, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    irows = np.zeros((len(uniq), backend.IMG_DESC_I), np.int64)
    frows = np.zeros((len(uniq), backend.IMG_DESC_F), np.float32)
    for u, (H, W, C) in enumerate(uniq.tolist()):
        got = _plan_one(stages, H, W, C)
        if got is None:
            return None
        pre, (Hr, Wr), post, chan, gray_of, ops = got
        resize = (Hr, Wr) != (pre[2], pre[3])
        flags = (1 * pre[5] + 2 * pre[4] + 4 * post[5] + 8 * post[4]
                 + 16 * resize + 32 * (layout == "CHW"))
        irows[u, :17] = [0, H, W, C, pre[0], pre[1], pre[2], pre[3], flags,
                         Hr, Wr, post[0], post[1], post[2], post[3],
                         len(chan),
                         sum(c << (8 * k) for k, c in enumerate(chan))]
        irows[u, 17] = sum(c << (8 * k) for k, c in enumerate(gray_of))
        irows[u, 19] = len(ops)
        irows[u, 20] = sum(kind << (8 * j) for j, (kind, _) in enumerate(ops))
        frows[u, 0] = np.float32(pre[2]) / np.float32(Hr)
        frows[u, 1] = np.float32(pre[3]) / np.float32(Wr)
        for j, (_, vals) in enumerate(ops):
            frows[u, 2 + 8 * j:10 + 8 * j] = vals
    idesc = irows[inv] if n else irows[:0]
    fdesc = frows[inv] if n else frows[:0]
    src_size = sh[:, 0] * sh[:, 1] * sh[:, 2]
    if src_off is None:
        src_off = np.concatenate([[0], np.cumsum(src_size)[:-1]]) if n \
            else np.zeros(0, np.int64)
    src_off = np.asarray(src_off, dtype=np.int64)
    src_numel = int((src_off + src_size).max()) if n else 0
    Ho, Wo, Co = idesc[:, 13], idesc[:, 14], idesc[:, 15]
    out_size = Ho * Wo * Co
    step = (out_size + 3) // 4 * 4 if out_u8 else out_size
    out_off = np.concatenate([[0], np.cumsum(step)[:-1]]).astype(np.int64) \
        if n else np.zeros(0, np.int64)
    idesc[:, 0], idesc[:, 18] = src_off, out_off
    work = np.concatenate([[0], np.cumsum(
        backend.image_work_items(Ho, Wo))]).astype(np.int64)
    if layout == "CHW":
        out_shapes = list(zip(Co.tolist(), Ho.tolist(), Wo.tolist()))
    else:
        out_shapes = list(zip(Ho.tolist(), Wo.tolist(), Co.tolist()))
    return ImagePlan(
        torch.from_numpy(np.ascontiguousarray(idesc)),
        torch.from_numpy(np.ascontiguousarray(fdesc)),
        torch.from_numpy(work), src_off, src_numel, out_off, out_shapes,
        int(step.sum()), torch.uint8 if dtype == np.uint8 else torch.float32,
        torch.uint8 if out_u8 else torch.float32)


def _transform_fused(vals, stages, keep_u8):
    """The column through one image_preprocess launch — pack into one
    (pinned) buffer, one H2D copy, one launch, one D2H copy, numpy views per
    row — or None when the column or the stages do not fit a plan."""
    from ..ops import backend
    from ..utils.devices import default_device
    if not len(vals) or not all(isinstance(v, np.ndarray) for v in vals):
        return None
    dtype = vals[0].dtype
    if dtype not in (np.uint8, np.float32) or not all(
            v.dtype == dtype and v.ndim in (2, 3) for v in vals):
        return None
    shapes = [(v.shape[0], v.shape[1], v.shape[2] if v.ndim == 3 else 1)
              for v in vals]
    plan = compile_image_plan(stages, shapes, dtype,
                              "uint8" if keep_u8 else "float32", "HWC")
    if plan is None:
        return None
    device = default_device("auto")
    src = torch.empty(plan.src_numel, dtype=plan.src_dtype,
                      pin_memory=device.type == "cuda")
    flat = src.numpy()
    for v, off in zip(vals, plan.src_off.tolist()):
        flat[off:off + v.size] = v.reshape(-1)
    out = torch.empty(plan.out_numel, dtype=plan.out_dtype, device=device)
    backend.image_preprocess(src.to(device, non_blocking=True), plan.idesc,
                             plan.fdesc, plan.work_off, out)
    host = out.cpu().numpy()
    return [host[off:off + h * w * c].reshape(h, w, c)
            for off, (h, w, c) in zip(plan.out_off.tolist(), plan.out_shapes)]


@register
class ImageTransformer(Transformer):
    """Stage-list image pipeline. Stages added with fluent helpers
    (ImageTransformer.scala:42-225) or via the ``stages`` param."""
    inputCol = Param("inputCol", "image column", "image")
    outputCol = Param("outputCol", "output image column", "out_image")
    stages = Param("stages", "ordered op list", None, toList)
    outputType = Param("outputType", "uint8|float", "uint8", toString)
    fused = Param("fused", "run stage lists that fit one plan (crops/flips, "
                  "one resize, colour, threshold, normalize) as a single "
                  "fused kernel launch over a column of any mix of shapes",
                  False, toBool)

    def _add(self, **stage):
        stages = list(self.get("stages") or [])
        stages.append(stage)
        self.set("stages", stages)
        return self

    def resize(self, height: int, width: int):
        return self._add(op="resize", height=height, width=width)

    def crop(self, x: int, y: int, height: int, width: int):
        return self._add(op="crop", x=x, y=y, height=height, width=width)

    def flip(self, flipCode: int = 1):
        return self._add(op="flip", flipCode=flipCode)

    def colorFormat(self, format: str):
        return self._add(op="colorFormat", format=format)

    def blur(self, height: int, width: int):
        return self._add(op="blur", height=height, width=width)

    def gaussianKernel(self, apertureSize: int, sigma: float):
        return self._add(op="gaussianKernel", apertureSize=apertureSize,
                         sigma=sigma)

    def threshold(self, threshold: float, maxVal: float = 255.0,
                  thresholdType: str = "binary"):
        return self._add(op="threshold", threshold=threshold, maxVal=maxVal,
                         thresholdType=thresholdType)

    def normalize(self, mean, std):
        return self._add(op="normalize", mean=mean, std=std)

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        from ..utils.devices import default_device
        stages = self.get("stages") or []
        keep_u8 = (self.get("outputType") == "uint8"
                   and not any(s["op"] == "normalize" for s in stages))
        vals = df[self.get("inputCol")].to_numpy()
        if self.get("fused"):
            outs = _transform_fused(vals, stages, keep_u8)
            if outs is not None:
                out = df.copy()
                out[self.get("outputCol")] = outs
                return out
        outs = []
        # uniform-shape batches run each op as one device launch
        uniform = (len(vals) > 1 and all(
            isinstance(v, np.ndarray) and v.shape == vals[0].shape
            for v in vals))
        if uniform:
            device = default_device("auto")
            chunk = max(1, int((1 << 28) / max(1, vals[0].size * 4)))
            for s0 in range(0, len(vals), chunk):
                t = torch.from_numpy(
                    np.stack(vals[s0:s0 + chunk])).float().to(device)
                if t.ndim == 3:
                    t = t.unsqueeze(-1)
                for st in stages:
                    t = _apply_stage_batched(t, st)
                if keep_u8:
                    a = t.clamp(0, 255).cpu().numpy().astype(np.uint8)
                else:
                    a = t.cpu().numpy()
                outs.extend(list(a))
        else:
            for img in vals:
                t = _to_tensor(img)
                for st in stages:
                    t = _apply_stage(t, st)
                outs.append(_to_array(t, keep_u8))
        out = df.copy()
        out[self.get("outputCol")] = outs
        return out


@register
class ImageSetAugmenter(Transformer):
    """Dataset augmentation by flips (ImageSetAugmenter.scala:18): emits the
    original rows plus flipped copies."""
    inputCol = Param("inputCol", "image column", "image")
    outputCol = Param("outputCol", "output column", "image")
    flipLeftRight = Param("flipLeftRight", "add LR flips", True)
    flipUpDown = Param("flipUpDown", "add UD flips", False)

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        frames = []
        base = df.copy()
        base[self.get("outputCol")] = df[self.get("inputCol")]
        frames.append(base)
        if self.get("flipLeftRight"):
            f = df.copy()
            f[self.get("outputCol")] = [np.ascontiguousarray(np.asarray(v)[:, ::-1])
                                        for v in df[self.get("inputCol")]]
            frames.append(f)
        if self.get("flipUpDown"):
            f = df.copy()
            f[self.get("outputCol")] = [np.ascontiguousarray(np.asarray(v)[::-1])
                                        for v in df[self.get("inputCol")]]
            frames.append(f)
        return pd.concat(frames, ignore_index=True)


@register
class ResizeImageTransformer(Transformer):
    """Standalone resize (image/ResizeImageTransformer.scala): bilinear
    resize to (height, width), preserving dtype."""
    inputCol = Param("inputCol", "image column", "image")
    outputCol = Param("outputCol", "output column", "image")
    height = Param("height", "target height", 224, toInt)
    width = Param("width", "target width", 224, toInt)
    fused = Param("fused", "resize the whole column, of any mix of shapes, "
                  "in a single fused kernel launch", False, toBool)

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        h, w = self.get("height"), self.get("width")
        out = df.copy()
        if self.get("fused"):
            vals = df[self.get("inputCol")].to_numpy()
            outs = _transform_fused(
                vals, [{"op": "resize", "height": h, "width": w}],
                len(vals) > 0 and getattr(vals[0], "dtype", None) == np.uint8)
            if outs is not None:
                out[self.get("outputCol")] = outs
                return out
        out[self.get("outputCol")] = [
            _to_array(_apply_stage(_to_tensor(np.asarray(v)),
                                   {"op": "resize", "height": h, "width": w}),
                      np.asarray(v).dtype == np.uint8)
            for v in df[self.get("inputCol")]]
        return out


@register
class UnrollImage(Transformer):
    """Image → flat float vector in CHANNEL-MAJOR (CHW) order with raw
    0-255 values — exactly the reference's rearrangement
    (image/UnrollImage.scala:30-55: index = h*W*C + w*C + c, emitted
    channel-by-channel)."""
    inputCol = Param("inputCol", "image column", "image")
    outputCol = Param("outputCol", "unrolled vector column", "unrolled")

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        out = df.copy()
        vecs = []
        for v in df[self.get("inputCol")]:
            a = np.asarray(v)
            if a.ndim == 2:
                a = a[:, :, None]
            vecs.append(np.ascontiguousarray(
                a.transpose(2, 0, 1)).reshape(-1).astype(np.float64))
        out[self.get("outputCol")] = vecs
        return out


@register
class UnrollBinaryImage(Transformer):
    """Encoded image bytes → decoded (+optional resize) → flat vector
    (image/UnrollImage.scala:186 UnrollBinaryImage)."""
    inputCol = Param("inputCol", "image-bytes column", "data")
    outputCol = Param("outputCol", "unrolled vector column", "unrolled")
    height = Param("height", "optional resize height (0 = keep)", 0, toInt)
    width = Param("width", "optional resize width (0 = keep)", 0, toInt)

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        from ..io_http.files import decode_image
        h, w = self.get("height"), self.get("width")
        out = df.copy()
        vecs = []
        for b in df[self.get("inputCol")]:
            img = decode_image(bytes(b))
            if h and w:
                img = _to_array(_apply_stage(
                    _to_tensor(img), {"op": "resize", "height": h,
                                      "width": w}), True)
            if img.ndim == 2:
                img = img[:, :, None]
            vecs.append(np.ascontiguousarray(
                img.transpose(2, 0, 1)).reshape(-1).astype(np.float64))
        out[self.get("outputCol")] = vecs
        return out
