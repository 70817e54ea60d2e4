"""The image_preprocess contract on the CPU: cpu_ref against today's
_apply_stage chain, against an exact-coordinate float64 oracle, the plan
compiler's refusals, the descriptor check and ImageTransformer(fused=True).

Bound of the resize test.  Values are 0..255; the window is (Hc, Wc).
  * Coordinates.  scale = f32(n_in)/f32(n_out) carries one rounding,
    scale*(d+0.5) another, the -0.5 a third; each is at most 2^-24 relative
    of a number below n_in, so src is off by at most 3*n_in*2^-24 per axis.
  * The interpolant is continuous and piecewise linear in src with slope at
    most 255 per unit — also where floor(src) flips to the next tap pair
    (both pairs give the same value there) and at the clamped far edge
    (both taps are the last sample).  A coordinate error e therefore moves
    the value by at most 255*e: 255*3*(Hc+Wc)*2^-24 for both axes.
  * The blend: l1 = src - i0 is exact (Sterbenz) or one rounding, l0 one
    more, then three products and sums per line and three for the column —
    about 10 roundings of values <= 255, each <= 255*2^-24.
  Sum: (3*(Hc+Wc) + 10)*2^-24*255 <= B = (4*(Hc+Wc) + 16)*2^-24*255.
A following normalize (v/255 - mean)/std divides the error by 255*|std| and
adds a rounding of v/255 (<= 2^-24), of the difference and of the quotient
(each <= 2^-24*(1+|mean|) before the division by |std|):
  B_norm = (B/255 + 3*2^-24*(1+|mean|)) / |std|.
Worst observed share of the bound on the shapes below: 0.221 of B and 0.220
of B_norm (both at 640x480 -> 224x224, float32 source)."""
import numpy as np
import pandas as pd
import pytest
import torch

from mmlspark_amd.models.images import (ImageTransformer,
                                        ResizeImageTransformer,
                                        compile_image_plan)
from mmlspark_amd.ops import backend

from . import image_preprocess_cases as cases
from .image_preprocess_cases import (color, crop, flip, normalize, resize,
                                     threshold)

RESIZE_SHAPES = [((1, 1), (3, 3)), ((2, 2), (5, 5)), ((7, 7), (3, 3)),
                 ((64, 48), (33, 65)), ((300, 200), (224, 224)),
                 ((31, 500), (7, 1000)), ((640, 480), (224, 224))]
EPS = 2.0 ** -24


# ------------------------------------------------- 1. plans without a resize
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("case", cases.no_resize_cases(),
                         ids=lambda c: c[0])
def test_no_resize_plan_equals_apply_stage_chain(case, dtype):
    _, stages, shapes = case
    rng = np.random.default_rng(11)
    imgs = [cases.rand_image(rng, *s, dtype=dtype) for s in shapes]
    for im in imgs:             # samples exactly at and beside the thresholds
        im.reshape(-1)[:4] = (127, 128, 100, 50)
    for out_type in ("uint8", "float32"):
        got, _ = cases.run_plans([(stages, "HWC", imgs)], out_type)
        for g, im in zip(got, imgs):
            ref = cases.apply_chain(im, stages, out_type == "uint8")
            assert g.dtype == ref.dtype and g.shape == ref.shape
            assert np.array_equal(g, ref, equal_nan=True)


def test_chw_layout_is_the_transposed_result():
    rng = np.random.default_rng(12)
    imgs = [cases.rand_image(rng, 5, 7, 3), cases.rand_image(rng, 2, 3, 3)]
    st = [flip(1), normalize([0.4, 0.5, 0.6], [0.2, 0.3, 0.4])]
    hwc, _ = cases.run_plans([(st, "HWC", imgs)], "float32")
    chw, _ = cases.run_plans([(st, "CHW", imgs)], "float32")
    for a, b in zip(hwc, chw):
        assert np.array_equal(a.transpose(2, 0, 1), b)


# ------------------------------------------------ 2. resize against the oracle
@pytest.mark.parametrize("src_hw,dst_hw", RESIZE_SHAPES)
def test_resize_within_bound_of_exact_oracle(src_hw, dst_hw):
    rng = np.random.default_rng(13)
    (Hc, Wc), (Hr, Wr) = src_hw, dst_hw
    B = (4 * (Hc + Wc) + 16) * EPS * 255
    assert B < 0.5
    for dtype in (np.uint8, np.float32):
        im = cases.rand_image(rng, Hc, Wc, 3, dtype)
        if dtype == np.float32:
            im = np.clip(im, 0, 255)
        (got,), _ = cases.run_plans([([resize(Hr, Wr)], "HWC", [im])],
                                    "float32")
        ref = cases.oracle_resize(im, Hr, Wr)
        share = np.abs(got - ref).max() / B
        print("resize %s->%s %s: %.3f of B" % (src_hw, dst_hw,
                                               np.dtype(dtype).name, share))
        assert share <= 1.0
    # the same with a normalize behind it
    mean = np.array([0.485, 0.456, 0.406], np.float32)
    std = np.array([0.229, 0.224, 0.225], np.float32)
    st = [resize(Hr, Wr), normalize(mean.tolist(), std.tolist())]
    (got,), _ = cases.run_plans([(st, "HWC", [im])], "float32")
    ref = (cases.oracle_resize(im, Hr, Wr) / 255.0
           - mean.astype(np.float64)) / std.astype(np.float64)
    Bn = (B / 255 + 3 * EPS * (1 + mean.astype(np.float64))) / std
    share = (np.abs(got - ref) / Bn).max()
    print("resize+normalize %s->%s: %.3f of B_norm" % (src_hw, dst_hw, share))
    assert share <= 1.0


def test_resize_with_windows_and_flips_against_oracle():
    """Pre-crop/flip, resize, post-crop/flip: the oracle applies the same
    geometry with numpy slicing around its float64 resize."""
    rng = np.random.default_rng(14)
    im = cases.rand_image(rng, 20, 30, 3)
    st = [crop(2, 3, 15, 40), flip(1), resize(9, 50), flip(0),
          crop(5, 1, 6, 30), flip(-1)]
    (got,), _ = cases.run_plans([(st, "HWC", [im])], "float32")
    win = im[3:18, 2:30][:, ::-1]
    ref = cases.oracle_resize(win, 9, 50)[::-1][1:7, 5:35][::-1, ::-1]
    assert got.shape == ref.shape == (6, 30, 3)
    B = (4 * (15 + 28) + 16) * EPS * 255
    assert np.abs(got - ref).max() <= B


# ------------------------------------ 3. against today's torch path, resized
def test_resize_uint8_within_one_of_torch_path():
    rng = np.random.default_rng(15)
    differ = total = 0
    for (Hc, Wc), (Hr, Wr) in RESIZE_SHAPES:
        im = cases.rand_image(rng, Hc, Wc, 3)
        st = [resize(Hr, Wr)]
        (got,), _ = cases.run_plans([(st, "HWC", [im])], "uint8")
        ref = cases.apply_chain(im, st, True)
        d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        assert d.max() <= 1, (Hc, Wc, Hr, Wr, int(d.max()))
        differ += int((d != 0).sum())
        total += d.size
    print("uint8 samples differing from the torch path: %d of %d (%.4f %%)"
          % (differ, total, 100.0 * differ / total))


# ----------------------------------------------------------- 4. plan compiler
REFUSED = [
    ("blur", [{"op": "blur", "height": 3, "width": 3}]),
    ("gaussian", [{"op": "gaussianKernel", "apertureSize": 3, "sigma": 1.0}]),
    ("two_resizes", [resize(8, 8), resize(4, 4)]),
    ("gray_before_resize", [color("gray"), resize(4, 4)]),
    ("threshold_before_resize", [threshold(9.0, "binary"), resize(4, 4)]),
    ("normalize_before_resize", [normalize([0.5], [0.5]), resize(4, 4)]),
    ("negative_crop_origin", [crop(-1, 0, 3, 3)]),
    ("crop_leaves_nothing", [crop(6, 0, 3, 3)]),
    ("five_pointwise_ops", [threshold(float(t), "tozero") for t in range(5)]),
]


@pytest.mark.parametrize("name,stages", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_stage_list_keeps_todays_result(name, stages):
    shapes = [(6, 6, 3), (5, 6, 3)]
    assert compile_image_plan(stages, shapes, np.uint8, "uint8",
                              "HWC") is None
    rng = np.random.default_rng(16)
    df = pd.DataFrame({"image": [cases.rand_image(rng, *s) for s in shapes]})
    a = ImageTransformer(stages=stages, fused=True).transform(df)
    b = ImageTransformer(stages=stages).transform(df)
    for x, y in zip(a["out_image"], b["out_image"]):
        assert x.dtype == y.dtype and np.array_equal(x, y)


def test_plan_groups_by_shape_and_packs_outputs():
    shapes = [(5, 7, 3), (9, 4, 1), (5, 7, 3)]
    plan = compile_image_plan([crop(1, 1, 6, 5)], shapes, np.uint8, "uint8",
                              "HWC")
    assert plan.out_shapes == [(4, 5, 3), (6, 3, 1), (4, 5, 3)]
    assert plan.src_off.tolist() == [0, 105, 141]
    assert plan.out_off.tolist() == [0, 60, 80]          # dword-aligned
    assert plan.out_numel == 140
    same = [k for k in range(24) if k not in (0, 18)]
    assert torch.equal(plan.idesc[0, same], plan.idesc[2, same])
    assert plan.work_off.tolist() == [0, 1, 2, 3]
    assert compile_image_plan([], [(5, 5, 5)], np.uint8, "uint8",
                              "HWC") is None             # > 4 channels
    assert compile_image_plan([], [(5, 5, 3)], np.float64, "uint8",
                              "HWC") is None


# ------------------------------------------------ 5. check_image_descriptors
def _valid():
    plan = compile_image_plan(
        [crop(1, 0, 5, 5), resize(4, 6), color("gray"),
         threshold(3.0, "trunc")], [(6, 7, 3), (5, 5, 3)], np.uint8,
        "uint8", "HWC")
    src = torch.zeros(plan.src_numel, dtype=torch.uint8)
    out = torch.zeros(plan.out_numel, dtype=torch.uint8)
    return [src, plan.idesc.clone(), plan.fdesc.clone(),
            plan.work_off.clone(), out]


def _set(col, value, row=0):
    def edit(a):
        a[1][row, col] = value
    return edit


def _replace(k, fn):
    def edit(a):
        a[k] = fn(a[k])
    return edit


def _unaligned(a):
    a[4] = torch.zeros(52, dtype=torch.uint8)
    a[1][0, 18], a[1][1, 18] = 1, 28


BROKEN = [
    ("src_dtype", _replace(0, lambda t: t.to(torch.int32)), "flat contig"),
    ("out_dtype", _replace(4, lambda t: t.to(torch.float64)), "flat contig"),
    ("out_not_contiguous", _replace(4, lambda t: t.repeat(2)[::2]),
     "flat contig"),
    ("idesc_dtype", _replace(1, lambda t: t.to(torch.int32)), "CPU int64"),
    ("fdesc_dtype", _replace(2, lambda t: t.double()), "CPU float32"),
    ("work_off_shape", _replace(3, lambda t: t[:-1].clone()), "do not agree"),
    ("src_extent", _set(0, 130, row=1), "past the source buffer"),
    ("src_offset_negative", _set(0, -1), "past the source buffer"),
    ("pre_window_outside", _set(5, 3), "pre-window"),
    ("pre_window_negative", _set(4, -1), "pre-window"),
    ("copy_path_size_mismatch", _set(8, 0), "copy path"),
    ("scale_not_exact", lambda a: a[2].__setitem__((0, 0), 1.3), "scale"),
    ("post_window_outside", _set(11, 1), "post-window"),
    ("gray_channel_id", _set(17, 3 << 16), "channel map"),
    ("channel_code", _set(16, 5), "channel map"),
    ("source_channels", _set(3, 5), "channel count"),
    ("op_code", _set(20, 6), "op table"),
    ("op_count", _set(19, 5), "op table"),
    ("flag_bits", _set(8, 64 + 16), "flag bits"),
    ("out_extent", _set(18, 28, row=1), "past the output buffer"),
    ("out_overlap", _set(18, 0, row=1), "overlap"),
    ("out_not_dword_aligned", _unaligned, "dword"),
    ("work_off_not_prefix_sum", lambda a: a[3].__setitem__(1, 2),
     "prefix sum"),
    ("dimension_limit", _set(1, 32769), "dimension"),
]


@pytest.mark.parametrize("name,edit,msg", BROKEN, ids=[b[0] for b in BROKEN])
def test_check_image_descriptors_rejects(name, edit, msg):
    backend.check_image_descriptors(*_valid())          # the base passes
    args = _valid()
    edit(args)
    with pytest.raises(ValueError, match="image_preprocess: .*" + msg):
        backend.image_preprocess(*args)


def test_empty_batch_on_cpu():
    got, flat = cases.run_plans([], "uint8")
    assert got == [] and flat.size == 0


# ------------------------------------------- 6. ImageTransformer(fused=True)
def _mixed_column(rng, dtype=np.uint8):
    imgs = [cases.rand_image(rng, h, w, c, dtype) for h, w, c in
            [(30, 40, 3), (17, 9, 3), (40, 30, 3), (30, 40, 3), (8, 64, 3)]]
    return pd.DataFrame({"image": imgs})


def test_image_transformer_fused_mixed_column_cpu():
    rng = np.random.default_rng(17)
    df = _mixed_column(rng)
    t = ImageTransformer(fused=True).crop(2, 1, 28, 36).resize(12, 10) \
        .flip(1)
    out = t.transform(df)["out_image"]
    ref = ImageTransformer().crop(2, 1, 28, 36).resize(12, 10).flip(1) \
        .transform(df)["out_image"]
    for g, r in zip(out, ref):
        assert g.shape == r.shape == (12, 10, 3) and g.dtype == np.uint8
        assert np.abs(g.astype(np.int16) - r.astype(np.int16)).max() <= 1
    # a normalize makes the output float32; ragged outputs keep their shapes
    t = ImageTransformer(fused=True).crop(0, 0, 20, 20).colorFormat("gray") \
        .normalize([0.5], [0.25])
    out = list(t.transform(df)["out_image"])
    assert [o.shape for o in out] == [(20, 20, 1), (17, 9, 1), (20, 20, 1),
                                      (20, 20, 1), (8, 20, 1)]
    assert all(o.dtype == np.float32 for o in out)
    ref = ImageTransformer().crop(0, 0, 20, 20).colorFormat("gray") \
        .normalize([0.5], [0.25]).transform(df)["out_image"]
    for g, r in zip(out, ref):
        assert np.array_equal(g, r)
    # 2-D cells are one-channel images
    df2 = pd.DataFrame({"image": [im[:, :, 0].copy() for im in df["image"]]})
    out = ImageTransformer(fused=True).flip(0).transform(df2)["out_image"]
    for g, im in zip(out, df2["image"]):
        assert np.array_equal(g, im[::-1, :, None])


def test_image_transformer_fused_float32_column_and_output_type():
    rng = np.random.default_rng(18)
    df = _mixed_column(rng, np.float32)
    st = [threshold(100.0, "tozero_inv")]
    for otype, dt in (("uint8", np.uint8), ("float", np.float32)):
        got = ImageTransformer(stages=st, fused=True, outputType=otype) \
            .transform(df)["out_image"]
        ref = ImageTransformer(stages=st, outputType=otype) \
            .transform(df)["out_image"]
        for g, r in zip(got, ref):
            assert g.dtype == r.dtype == dt and np.array_equal(g, r)


def test_resize_image_transformer_fused_keeps_dtype():
    rng = np.random.default_rng(19)
    for dtype in (np.uint8, np.float32):
        df = _mixed_column(rng, dtype)
        got = ResizeImageTransformer(height=11, width=13, fused=True) \
            .transform(df)["image"]
        ref = ResizeImageTransformer(height=11, width=13) \
            .transform(df)["image"]
        for g, r in zip(got, ref):
            assert g.shape == r.shape == (11, 13, 3) and g.dtype == dtype
            if dtype == np.uint8:
                assert np.abs(g.astype(np.int16)
                              - r.astype(np.int16)).max() <= 1
            else:
                assert np.abs(g - r).max() <= 2 * (4 * 80 + 16) * EPS * 340
    # a float64 column does not fit a plan: today's path, today's result
    df = pd.DataFrame({"image": [np.ones((4, 4, 3)), np.ones((5, 4, 3))]})
    got = ResizeImageTransformer(height=2, width=2, fused=True).transform(df)
    assert all(g.shape == (2, 2, 3) for g in got["image"])
