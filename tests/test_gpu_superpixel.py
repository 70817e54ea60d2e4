"""superpixel_kernels.hip against float64 numpy references."""
import numpy as np
import pandas as pd
import pytest
import torch

from mmlspark_amd.explainers.lime import ImageLIME, SuperpixelTransformer
from mmlspark_amd.explainers.sampler import slic_superpixels
from mmlspark_amd.explainers.shap import ImageSHAP
from mmlspark_amd.models.image_featurizer import TorchModel, _unit_lut
from mmlspark_amd.ops import backend

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
# ragged edge (K = 35), K = 16, K = 80, K = 120, and a gray (H, W) image
SLIC_CASES = [((37, 53, 3), 8), ((64, 64, 3), 16), ((48, 40, 3), 5),
              ((96, 80, 3), 8), ((37, 53), 8)]


def noise(shape, dtype=np.uint8):
    return np.random.default_rng(0).integers(2, 256, size=shape).astype(dtype)


def features64(img, cell, mod=10.0):
    h, w = img.shape[:2]
    rgb = np.broadcast_to(img.reshape(h, w, -1), (h, w, 3)).astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.concatenate([rgb / mod, yy[..., None] / cell,
                           xx[..., None] / cell], axis=2).reshape(-1, 5)


def test_one_iteration_matches_float64():
    """Five iterations of the float64 trajectory; at each, the kernel gets the
    float64 centres rounded to float32 and runs one iteration on the whole
    column (mixed sizes and cell sizes, one call).

    Labels.  The kernel's distance is fl(sum_i fl(fl(p_i - c_i)^2)) with p_i
    a float32 feature and c_i a rounded centre, each within relative u = 2^-24
    of the float64 value.  To first order the difference d_i is off by at most
    u (|p_i| + |c_i| + |d_i|), its square by 2 |d_i| times that plus u d_i^2
    for the multiply, and the four additions add 4 u D.  So the float32
    distance lies within E = u (sum_i (2 |d_i| (|p_i| + |c_i| + |d_i|) +
    d_i^2) + 4 D) of D (times 1.001 for the second-order terms), and the
    kernel must pick the float64 argmin wherever D_best + E_best is below
    D_k - E_k for every other k.  Those pixels are checked; at most 1 % may
    fall outside (exact ties of the grid-symmetric start are among them).

    Centres.  The sums are exact integers, so the returned centre is the
    float64 mean over the kernel's own labels up to the divide, the scale and
    the rounding to float32: within 4 float32 ulp.  Cluster 7 of the fourth
    image starts far away, stays empty and must come back bit for bit."""
    imgs = [noise(s) for s, _ in SLIC_CASES]
    cells = [c for _, c in SLIC_CASES]
    feats = [features64(a, c) for a, c in zip(imgs, cells)]
    ctrs = []
    for a, c, f in zip(imgs, cells, feats):
        gy = np.arange(c // 2, a.shape[0], c)
        gx = np.arange(c // 2, a.shape[1], c)
        ctrs.append(f[(gy[:, None] * a.shape[1] + gx[None]).ravel()].copy())
    assert [len(c) for c in ctrs] == [35, 16, 80, 120, 35]
    ctrs[3][7] = 1e4
    dev_imgs = [torch.from_numpy(a).to(DEV) for a in imgs]
    for it in range(5):
        start = [c.astype(np.float32) for c in ctrs]
        labels, out = backend.slic_segment(
            dev_imgs, cells, 10.0, 1,
            centers=[torch.from_numpy(c).to(DEV) for c in start])
        for i, (f, c) in enumerate(zip(feats, ctrs)):
            d = f[:, None, :] - c[None]
            D = (d * d).sum(-1)
            E = 1.001 * U * ((2 * np.abs(d) * (np.abs(f[:, None]) + np.abs(c[None])
                                              + np.abs(d)) + d * d).sum(-1)
                             + 4 * D)
            rows, best = np.arange(len(f)), D.argmin(1)
            low = D - E
            low[rows, best] = np.inf
            sure = low.min(1) > (D + E)[rows, best]
            got = labels[i].cpu().numpy().ravel()
            print("iteration %d image %d: %.3f %% of pixels not checked"
                  % (it, i, 100 * (1 - sure.mean())))
            assert labels[i].shape == imgs[i].shape[:2]
            assert sure.mean() >= 0.99
            assert (got[sure] == best[sure]).all()

            def means(lab):
                cnt = np.bincount(lab, minlength=len(c))
                s = np.stack([np.bincount(lab, weights=f[:, q], minlength=len(c))
                              for q in range(5)], axis=1)
                return cnt > 0, s / np.maximum(cnt, 1)[:, None]
            full, want = means(got)
            have = out[i].cpu().numpy()
            ulp = np.spacing(np.abs(want[full]).astype(np.float32))
            assert (np.abs(have[full] - want[full]) <= 4 * ulp).all()
            assert np.array_equal(have[~full], start[i][~full])
            assert i != 3 or not full[7]
            full, want = means(best)       # the float64 trajectory goes on
            c[full] = want[full]


def test_five_iterations_with_default_seeds_match_numpy():
    """64 x 64, cell 16: the smallest float64 gap over all iterations is
    3.8e-3, far above any rounding, so the labels are slic_superpixels'."""
    img = noise((64, 64, 3))
    labels, centres = backend.slic_segment([torch.from_numpy(img).to(DEV)], 16,
                                           10.0, 5)
    assert centres[0].shape == (16, 5)
    assert np.array_equal(labels[0].cpu().numpy(), slic_superpixels(img, 16))


def test_more_centres_than_one_lds_chunk():
    """66 x 64, cell 2: K = 1056, two LDS chunks of centres and of sums.  The
    float32 contract (cpu_ref) does the kernel's operations in the kernel's
    order, every one correctly rounded, and the sums are exact: same bits."""
    img = torch.from_numpy(noise((66, 64, 3)))
    want_l, want_c = backend.slic_segment([img], 2, 10.0, 3)
    got_l, got_c = backend.slic_segment([img.to(DEV)], 2, 10.0, 3)
    assert got_c[0].shape == (1056, 5) and int(got_l[0].max()) >= 1024
    assert torch.equal(got_l[0].cpu(), want_l[0])
    assert torch.equal(got_c[0].cpu(), want_c[0])


def masked_ref(img, seg, states, fill, size):
    """float64: mask, / 255, CHW, then four taps at torch's float32 source
    coordinates (scale and coordinate are float32 by torch's definition; the
    weights and the blend are float64)."""
    h, w = img.shape[:2]
    rgb = np.broadcast_to(img.reshape(h, w, -1), (h, w, 3))
    x = np.where((states[:, seg] >= 0.5)[..., None], rgb, fill) / 255.0
    x = x.transpose(0, 3, 1, 2)
    if (h, w) == (size, size):
        return x

    def axis(n_in):
        s = np.float32(n_in) / np.float32(size) * (
            np.arange(size, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
        s = np.maximum(s, np.float32(0))
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        return i0, np.minimum(i0 + 1, n_in - 1), s.astype(np.float64) - i0
    y0, y1, ly = axis(h)
    x0, x1, lx = axis(w)
    top = x[:, :, y0][..., x0] * (1 - lx) + x[:, :, y0][..., x1] * lx
    bot = x[:, :, y1][..., x0] * (1 - lx) + x[:, :, y1][..., x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


@pytest.mark.parametrize("fill", [0, 128])
@pytest.mark.parametrize("shape,m,size", [
    ((23, 31, 3), 70, 16), ((23, 31, 3), 70, 40), ((23, 31, 3), 5, 40),
    ((16, 16), 5, 16), ((16, 16), 70, 16), ((16, 16), 70, 40)])
def test_masked_image_batch(shape, m, size, fill):
    """Without a resize the batch is lut[masked image] bit for bit.  With one,
    values lie in [0, 1] and at most six float32 roundings of at most 2^-24
    each enter a tap blend: 1e-6 absolute."""
    img = noise(shape)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    seg = (((yy // 3) * 11 + xx // 2) % m).astype(np.int32)
    states = (np.random.default_rng(1).random((37, m)) < 0.5).astype(np.float32)
    states[0], states[1] = 1, 0
    states[2:6] = np.eye(m, dtype=np.float32)[[0, m - 1, min(31, m - 1),
                                               min(32, m - 1)]]
    lut = _unit_lut(torch.device(DEV))
    got = backend.masked_image_batch(
        torch.from_numpy(img).to(DEV), torch.from_numpy(seg).to(DEV),
        backend.pack_states(states).to(DEV), fill, size, lut, m=m).cpu().numpy()
    want = masked_ref(img, seg, states, fill, size)
    assert got.shape == (37, 3, size, size) and got.dtype == np.float32
    if shape[:2] == (size, size):
        assert np.array_equal(got, lut.cpu().numpy()[(want * 255).round()
                                                     .astype(np.int64)])
    else:
        assert np.abs(got - want).max() <= 1e-6


class Functional(torch.nn.Module):
    """Two linear functionals of the input, summed in float64 per sample."""

    def __init__(self):
        super().__init__()
        w = torch.linspace(-1, 1, 3 * 64 * 64, dtype=torch.float64)
        self.register_buffer("w", torch.stack([w, w.flip(0) ** 2]))

    def forward(self, x):
        return (x.double().flatten(1) @ self.w.t()).float()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("explainer", [ImageLIME, ImageSHAP])
def test_explainers_match_the_sample_path(explainer, dtype):
    """uint8 takes the device path, float32 the sample path; either way the
    superpixels and the explanations are those with fusedSampling off."""
    df = pd.DataFrame({"image": [noise((64, 64, 3), dtype)]})
    model = TorchModel(Functional(), inputCol="image", outputCol="output",
                       device=DEV)
    off, on = (explainer(model=model, inputCol="image", targetCol="output",
                         targetClasses=[0, 1], numSamples=64, cellSize=16,
                         fusedSampling=f).transform(df) for f in (False, True))
    assert np.array_equal(on["superpixels"][0], off["superpixels"][0])
    assert on["superpixels"][0].dtype == off["superpixels"][0].dtype
    assert np.array_equal(on["explanation"][0], off["explanation"][0])


def test_superpixel_transformer_segments_a_column_on_the_device():
    imgs = [noise((64, 64, 3)), noise((37, 53))]
    out = SuperpixelTransformer(inputCol="image", cellSize=8, device=DEV) \
        .transform(pd.DataFrame({"image": imgs}))["superpixels"]
    for a, got in zip(imgs, out):
        want, _ = backend.slic_segment([torch.from_numpy(a).to(DEV)], 8)
        assert np.array_equal(got, want[0].cpu().numpy())
