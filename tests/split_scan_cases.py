"""Shared cases and float64 oracle of the split-finder tests (CPU and GPU
files).

The oracle is plain numpy float64 and shares nothing with cpu_ref or with the
kernel: per-feature, per-bin prefix sums, the validity test, the gain table
and a first-index arg-max (lowest feature, then lowest bin).

Family A holds integers and small dyadic fractions only, so every prefix sum
is exact in float32 in any summation order: GL/HL/CL must equal the oracle's
exactly, and candidates with the same prefix sums have bit-identical gains in
any arithmetic.  Family B holds real-valued g and h over mostly empty bins;
its tolerance is measured (B_GAIN_MEASURED below).

Every case is checked where it is built (check_margins): a candidate that is
not exactly tied with the best loses by more than the float32 error can
bridge, so the expected (feature, bin) is exact in both families.
"""
import functools

import numpy as np
import torch

NEG_INF = float("-inf")
U24 = 2.0 ** -24

# Family A margin: each of the three scores carries at most 5 float32
# roundings (|G|-l1, the square, H+l2, +1e-32, the division) and the two
# additions of the gain two more, so a float32 gain is off by at most about
# 7 * 2^-24 * (sc(L)+sc(R)+sc(P)); the margin is twice that, rounded up.
A_MARGIN = 16 * U24

# Family B tolerance, relative to sc(L)+sc(R)+sc(P) of the candidate.
# B_GAIN_MEASURED is the largest |gain_f32 - gain_f64| / (sc(L)+sc(R)+sc(P))
# that cpu_ref.split_scan (float32 torch on the CPU, sequential cumsum) shows
# against the oracle over the Family B cases below, rounded up to two digits
# (test_split_scan_ref.py re-measures it and fails if it is exceeded).  The
# GPU test allows 4x: room for the kernel's tree-shaped summation order and
# no more.  B_PREFIX_* is the same for the prefix sums GL / HL, relative to
# the feature's sum of |g| / of h.
B_GAIN_MEASURED = 1.1e-6      # measured 1.013e-6 (real_2x28x255_s1)
B_GAIN_BOUND = 4 * B_GAIN_MEASURED
B_PREFIX_MEASURED = 4.8e-8    # measured 4.79e-8
B_PREFIX_BOUND = 4 * B_PREFIX_MEASURED


# ------------------------------------------------------------------ oracle
def _score(G, H, l1, l2):
    a = np.maximum(np.abs(G) - l1, 0.0)
    return a * a / (H + l2 + 1e-32)


def oracle(hists, l1, l2, min_data, min_hess, nf_real, feat_mask=None):
    """float64 gain table of (nh, nf_pad, n_bins, 3) histograms.

    Returns a dict: gain (nh, nf_pad, n_bins) with -inf where no split is
    allowed, scale = sc(L)+sc(R)+sc(P), prefix (nh, nf_pad, n_bins, 3), and
    per histogram best = (gain, feature, bin) by first index — lowest
    feature, then lowest bin — or (-inf, None, None) with no valid split."""
    h = np.asarray(hists, dtype=np.float64)
    nh, nf_pad, nb, _ = h.shape
    l1, l2 = float(l1), float(l2)
    pre = np.cumsum(h, axis=2)
    tot = pre[:, :, -1:, :]
    GL, HL, CL = pre[..., 0], pre[..., 1], pre[..., 2]
    GR, HR, CR = (tot - pre)[..., 0], (tot - pre)[..., 1], (tot - pre)[..., 2]
    sL, sR = _score(GL, HL, l1, l2), _score(GR, HR, l1, l2)
    sP = _score(tot[..., 0], tot[..., 1], l1, l2)
    scale = sL + sR + sP
    gain = sL + sR - sP
    ok = ((CL >= min_data) & (CR >= min_data)
          & (HL >= min_hess) & (HR >= min_hess))
    ok[:, :, nb - 1] = False                       # never at the last bin
    live = np.arange(nf_pad) < nf_real             # pad features
    if feat_mask is not None:
        live &= np.asarray(feat_mask, dtype=bool)[:nf_pad]
    occupied = (h[..., 2] > 0).sum(axis=2)         # (nh, nf_pad)
    ok &= (live[None, :] & (occupied > 1))[:, :, None]
    gain = np.where(ok, gain, NEG_INF)
    best = []
    for i in range(nh):
        flat = gain[i].reshape(-1)
        j = int(np.argmax(flat))                   # first index of the max
        if flat[j] == NEG_INF:
            best.append((NEG_INF, None, None))
        else:
            best.append((float(flat[j]), j // nb, j % nb))
    return dict(gain=gain, scale=scale, prefix=pre, best=best)


# ------------------------------------------------------------------- cases
def _case(name, family, hists, l1=0.0, l2=0.0, min_data=1.0, min_hess=0.0,
          nf_real=None, feat_mask=None, expect=None):
    hists = np.ascontiguousarray(hists, dtype=np.float32)
    nh, nf_pad, nb, _ = hists.shape
    return dict(name=name, family=family, hists=hists, n_bins=nb,
                l1=float(l1), l2=float(l2), min_data=float(min_data),
                min_hess=float(min_hess),
                nf_real=nf_pad if nf_real is None else int(nf_real),
                feat_mask=None if feat_mask is None
                else np.asarray(feat_mask, dtype=bool),
                expect=expect)


def _blank(nh, nf_pad, nb):
    return np.zeros((nh, nf_pad, nb, 3), dtype=np.float64)


def _lumps(h, hi, f, *lumps):
    """lumps: (bin, g, h, count) — every other bin of the feature empty."""
    h[hi, f] = 0.0
    for b, g, hh, c in lumps:
        h[hi, f, b] = (g, hh, c)


def _pair(h, hi, f, a, b, g=8.0, hh=4.0, c=4.0):
    """+g in bin a, -g in bin b: G = 0, gain 2 g^2 / hh (l1 = l2 = 0) for
    every bin in a..b-1, all exactly tied; the first is a."""
    _lumps(h, hi, f, (a, g, hh, c), (b, -g, hh, c))


def _weak(h, hi, feats, nb):
    """Low-gain background (gain 0.5 at l1 = l2 = 0), split at bin 0."""
    for f in feats:
        _pair(h, hi, f, 0, nb - 1, g=1.0)


def _family_a():
    out = []

    # n_bins sweep: the best split at bin 0 and at bin n_bins - 2
    for nb in (2, 3, 63, 64, 65, 255, 256):
        h = _blank(2, 4, nb)
        for hi in range(2):
            _weak(h, hi, range(4), nb)
        if nb == 2:
            _pair(h, 0, 2, 0, 1)
            _pair(h, 1, 1, 0, 1)
            exp = [(2, 0), (1, 0)]
        else:
            _pair(h, 0, 2, 0, 1)
            _pair(h, 1, 1, nb - 2, nb - 1)
            exp = [(2, 0), (1, nb - 2)]
        out.append(_case("bins%d" % nb, "A", h, expect=exp))

    # the prefix at the last bin would win if it were allowed: l1 makes every
    # real split lose against the parent (gain < 0) while "everything left"
    # has gain exactly 0; min_data = min_hess = 0 lets the counts pass
    h = _blank(1, 4, 8)
    _lumps(h, 0, 0, (0, 5.0, 5.0, 5.0), (7, 5.0, 5.0, 5.0))      # gain -2.8
    _lumps(h, 0, 1, (0, 4.0, 5.0, 5.0), (7, 4.0, 5.0, 5.0))      # gain -2.0
    _lumps(h, 0, 2, (0, 6.0, 5.0, 5.0), (7, 5.0, 5.0, 5.0))      # gain -3.1
    _lumps(h, 0, 3, (0, 4.0, 5.0, 5.0), (7, 7.0, 5.0, 5.0))      # gain -2.3
    out.append(_case("last_bin", "A", h, l1=2.0, min_data=0.0,
                     expect=[(1, 0)]))

    # runs of empty bins: the tied set straddles each halving boundary of the
    # block arg-max; the first bin of the run is expected
    h = _blank(3, 4, 256)
    for hi, (a, b) in enumerate(((125, 131), (60, 70), (30, 40))):
        _weak(h, hi, range(4), 256)
        _pair(h, hi, hi + 1, a, b)
    out.append(_case("runs_mid", "A", h,
                     expect=[(1, 125), (2, 60), (3, 30)]))
    h = _blank(2, 4, 256)
    for hi in range(2):
        _weak(h, hi, range(4), 256)
    _pair(h, 0, 3, 0, 200)             # tied 0..199
    _pair(h, 1, 0, 127, 255)           # tied 127..254
    out.append(_case("runs_far", "A", h, expect=[(3, 0), (0, 127)]))

    # duplicate columns: the lowest feature wins
    for name, nf_pad, dup in (("dup_0_1", 8, (0, 1)),
                              ("dup_5_300", 304, (5, 300)),
                              ("dup_3_259", 260, (3, 259)),
                              ("dup_3_259_515", 516, (259, 515, 3))):
        h = _blank(1, nf_pad, 16)
        _weak(h, 0, range(nf_pad), 16)
        for f in dup:
            _lumps(h, 0, f, (2, 8.0, 4.0, 4.0), (5, -3.0, 2.0, 2.0),
                   (9, -5.0, 2.0, 2.0))
        out.append(_case(name, "A", h, expect=[(min(dup), 2)]))

    # three histograms, three winners, one thread owning several features
    h = _blank(3, 260, 16)
    for hi, f in enumerate((258, 0, 130)):
        _weak(h, hi, range(260), 16)
        _pair(h, hi, f, 3 + hi, 9)
    out.append(_case("three_hists", "A", h,
                     expect=[(258, 3), (0, 4), (130, 5)]))

    # masks and pad features; the excluded features would win by far
    def masked(name, nf_real, mask, exp):
        h = _blank(1, 8, 16)
        _weak(h, 0, range(8), 16)
        _pair(h, 0, 0, 2, 3, g=64.0)              # feature 0: gain 2048
        _pair(h, 0, 3, 4, 6, g=8.0)
        for f in (5, 6, 7):
            _pair(h, 0, f, 1, 2, g=128.0)         # pad candidates
        return _case(name, "A", h, nf_real=nf_real, feat_mask=mask,
                     expect=exp)

    m = np.ones(8, dtype=bool)
    m0 = m.copy()
    m0[0] = False
    out.append(masked("mask_f0", 5, m0, [(3, 4)]))
    out.append(masked("mask_all", 8, np.zeros(8, dtype=bool), [None]))
    out.append(masked("nf_real_1", 1, None, [(0, 2)]))
    out.append(masked("nf_real_pad_minus_3", 5, m, [(0, 2)]))
    out.append(masked("nf_real_pad", 8, None, [(5, 1)]))

    # no valid split anywhere: min_data above every count
    h = _blank(2, 4, 16)
    for hi in range(2):
        _weak(h, hi, range(4), 16)
        _pair(h, hi, 2, 3, 7)
    out.append(_case("no_valid", "A", h, min_data=1000.0,
                     expect=[None, None]))

    # one-occupied-bin features next to a real one.  At min_data 0 a
    # degenerate feature's "split" has gain exactly 0 and would beat the real
    # feature's best (negative under l1) if it were allowed.
    h = _blank(1, 4, 16)
    _lumps(h, 0, 0, (3, 50.0, 10.0, 10.0))
    _lumps(h, 0, 1, (0, 50.0, 10.0, 10.0))
    _pair(h, 0, 2, 5, 9)
    _lumps(h, 0, 3, (15, 50.0, 10.0, 10.0))
    out.append(_case("one_bin_min_data_1", "A", h, min_data=1.0,
                     expect=[(2, 5)]))
    h = _blank(1, 4, 16)
    _lumps(h, 0, 0, (3, 10.0, 10.0, 10.0))
    _lumps(h, 0, 1, (0, 10.0, 10.0, 10.0))
    _lumps(h, 0, 2, (0, 5.0, 5.0, 5.0), (15, 5.0, 5.0, 5.0))    # gain -2.8
    _lumps(h, 0, 3, (15, 10.0, 10.0, 10.0))
    out.append(_case("one_bin_min_data_0", "A", h, l1=2.0, min_data=0.0,
                     expect=[(2, 0)]))

    # boundary equality is accepted, one count / one step of h below is not:
    # feature 0 is the stronger split and sits just below the boundary,
    # feature 1 sits on it
    step = 2.0 ** -12
    h = _blank(2, 4, 16)
    _lumps(h, 0, 0, (2, 16.0, 4.0, 3.0), (6, -16.0, 4.0, 10.0))  # CL = 3
    _lumps(h, 0, 1, (2, 8.0, 4.0, 4.0), (6, -8.0, 4.0, 10.0))    # CL = 4
    _lumps(h, 1, 0, (2, 16.0, 4.0, 10.0), (6, -16.0, 4.0, 3.0))  # CR = 3
    _lumps(h, 1, 1, (2, 8.0, 4.0, 10.0), (6, -8.0, 4.0, 4.0))    # CR = 4
    out.append(_case("min_data_edge", "A", h, min_data=4.0,
                     expect=[(1, 2), (1, 2)]))
    h = _blank(2, 4, 16)
    _lumps(h, 0, 0, (2, 16.0, 0.5 - step, 5.0), (6, -16.0, 4.0, 5.0))
    _lumps(h, 0, 1, (2, 8.0, 0.5, 5.0), (6, -8.0, 4.0, 5.0))     # HL = 0.5
    _lumps(h, 1, 0, (2, 16.0, 4.0, 5.0), (6, -16.0, 0.5 - step, 5.0))
    _lumps(h, 1, 1, (2, 8.0, 4.0, 5.0), (6, -8.0, 0.5, 5.0))     # HR = 0.5
    out.append(_case("min_hess_edge", "A", h, min_hess=0.5,
                     expect=[(1, 2), (1, 2)]))

    # L1: |G| below l1 on one side (that score clamps to 0) ...
    h = _blank(1, 4, 16)
    _weak(h, 0, range(4), 16)
    _lumps(h, 0, 2, (1, 2.0, 4.0, 4.0), (8, -16.0, 4.0, 4.0))
    out.append(_case("l1_one_side", "A", h, l1=3.0, l2=0.5,
                     expect=[(2, 1)]))
    # ... and everywhere: every score is 0, every valid candidate ties at
    # gain 0, the first valid one is feature 0's first bin with CL >= 2
    h = _blank(1, 4, 16)
    _lumps(h, 0, 0, (1, 1.0, 4.0, 1.0), (3, -2.0, 4.0, 1.0),
           (9, 1.0, 4.0, 4.0))
    _lumps(h, 0, 1, (0, 2.0, 4.0, 3.0), (4, -1.0, 4.0, 3.0))
    _pair(h, 0, 2, 0, 15, g=2.0)
    _pair(h, 0, 3, 0, 15, g=1.0)
    out.append(_case("l1_everywhere", "A", h, l1=8.0, min_data=2.0,
                     expect=[(0, 3)]))
    # l2 = 0 with tiny but nonzero h
    tiny = 2.0 ** -20
    h = _blank(1, 4, 16)
    _weak(h, 0, range(4), 16)
    _lumps(h, 0, 1, (4, 8.0, tiny, 4.0), (7, -4.0, tiny, 4.0),
           (11, -2.0, 2 * tiny, 4.0))
    out.append(_case("l2_zero_tiny_h", "A", h, expect=[(1, 4)]))

    # mixed signs that cancel to G = 0 over three lumps
    h = _blank(1, 4, 64)
    _weak(h, 0, range(4), 64)
    _lumps(h, 0, 3, (10, 6.0, 2.0, 3.0), (20, -10.0, 2.0, 3.0),
           (63, 4.0, 2.0, 3.0))
    out.append(_case("cancel", "A", h, l2=1.0, expect=[(3, 10)]))

    # counts near 2^24: every prefix count stays exact in float32
    big = 2.0 ** 23
    h = _blank(1, 4, 16)
    _weak(h, 0, range(4), 16)
    _lumps(h, 0, 0, (0, 8.0, 4.0, 2 * big - 1), (5, -8.0, 4.0, 1.0))
    _lumps(h, 0, 1, (3, 8.0, 4.0, big), (4, -8.0, 4.0, big))
    out.append(_case("counts_2p24", "A", h, min_data=2.0,
                     expect=[(1, 3)]))
    return out


B_SHAPES = (((2, 28, 255), 26, (0, 1, 2)), ((1, 260, 64), 257, (3, 4, 5)))


def _family_b():
    out = []
    for (nh, nf_pad, nb), nf_real, seeds in B_SHAPES:
        for seed in seeds:
            gen = torch.Generator().manual_seed(seed)
            g = torch.randn(nh, nf_pad, nb, generator=gen)
            hh = torch.rand(nh, nf_pad, nb, generator=gen) + 0.01
            c = torch.randint(1, 50, (nh, nf_pad, nb), generator=gen).float()
            keep = (torch.rand(nh, nf_pad, nb, generator=gen) < 0.3).float()
            h = torch.stack([g * keep, hh * keep, c * keep], dim=-1).numpy()
            h = h + 0.0         # an emptied bin holds +0.0, never -0.0
            mask = np.ones(nf_pad, dtype=bool)
            mask[[3, 7]] = False
            out.append(_case("real_%dx%dx%d_s%d" % (nh, nf_pad, nb, seed),
                             "B", h, l1=0.1, l2=0.5, min_data=3.0,
                             min_hess=1e-3, nf_real=nf_real, feat_mask=mask))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case, in a fixed order; read-only."""
    return {c["name"]: c for c in _family_a() + _family_b()}


CASE_NAMES = tuple(cases())
A_NAMES = tuple(n for n, c in cases().items() if c["family"] == "A")
B_NAMES = tuple(n for n, c in cases().items() if c["family"] == "B")


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's result for a case, computed once; read-only."""
    c = cases()[name]
    return oracle(c["hists"], c["l1"], c["l2"], c["min_data"], c["min_hess"],
                  c["nf_real"], c["feat_mask"])


def margin_of(name):
    c = cases()[name]
    return A_MARGIN if c["family"] == "A" else 2 * B_GAIN_BOUND


def check_margins(name):
    """The builder's assertions, in float64: every candidate is either tied
    with the best through identical prefix sums, or through every score
    being 0 (either way its gain is bit-identical in any arithmetic), or
    loses by more than margin * scale; no validity test
    hangs on a rounding of h; the stated expectation is the oracle's."""
    c = cases()[name]
    o = expected(name)
    h64 = c["hists"].astype(np.float64)
    if c["family"] == "A":
        # exact in float32 in any order: dyadic, and the sum of magnitudes
        # needs no more than 24 bits above its smallest unit
        for k in range(3):
            v = np.abs(h64[..., k])
            nz = np.unique(v[v > 0])
            if nz.size:
                lsb = min(_lowest_bit(x) for x in nz)
                assert v.sum(axis=2).max() / lsb <= 2.0 ** 24, name
    margin = margin_of(name)
    for i, (bg, bf, bb) in enumerate(o["best"]):
        want = None if c["expect"] is None else c["expect"][i]
        if bf is None:
            assert c["expect"] is None or want is None, name
            continue
        if c["expect"] is not None:
            assert want == (bf, bb), (name, i, want, (bf, bb))
        gain, scale, pre = o["gain"][i], o["scale"][i], o["prefix"][i]
        tot = pre[:, -1, :]
        finite = gain > NEG_INF
        same = (np.all(pre == pre[bf, bb], axis=-1)
                & np.all(tot == tot[bf], axis=-1)[:, None])
        tied = finite & (gain == bg)
        same |= (scale == 0.0) & (scale[bf, bb] == 0.0)
        assert np.all(same[tied]), (name, i, "tie between unlike candidates")
        rest = finite & ~tied
        need = margin * np.maximum(scale, scale[bf, bb])
        assert np.all((bg - gain)[rest] > need[rest]), (name, i, "margin")
        if c["family"] == "B":
            # min_hess is never decided by a rounding: wherever the counts
            # pass, HL and HR are far from it
            cl = pre[..., 2]
            cr = tot[:, None, 2] - cl
            cnt = (cl >= c["min_data"]) & (cr >= c["min_data"])
            hl = pre[..., 1]
            hr = tot[:, None, 1] - hl
            gap = np.minimum(np.abs(hl - c["min_hess"]),
                             np.abs(hr - c["min_hess"]))
            assert np.all(gap[cnt] > 1e-3), (name, i, "min_hess edge")


def _lowest_bit(x):
    """Largest power of two that divides the dyadic number x > 0."""
    m, e = np.frexp(x)
    m = int(m * 2 ** 53)
    return float((m & -m)) * 2.0 ** (int(e) - 53)


def torch_inputs(name, device="cpu"):
    c = cases()[name]
    hists = torch.from_numpy(c["hists"]).to(device)
    mask = (None if c["feat_mask"] is None
            else torch.from_numpy(c["feat_mask"]).to(device))
    return hists, mask


def run(fn, name, device="cpu"):
    """fn is backend.split_scan or cpu_ref.split_scan; returns (nh, 6)."""
    c = cases()[name]
    hists, mask = torch_inputs(name, device)
    out = fn(hists, c["n_bins"], c["l1"], c["l2"], c["min_data"],
             c["min_hess"], 0.0, c["nf_real"], mask)
    return out.cpu().numpy()


def check_result(out, name, gain_tol, prefix_tol):
    """out (nh, 6) against the oracle.  The (feature, bin) must be exact;
    the gain within gain_tol * scale, GL / HL within prefix_tol * (sum |g| /
    sum h of the feature), CL exact (tolerances 0: exact equality with the
    oracle's float64 values, which are float32 numbers in Family A).  Returns
    the worst (gain error / scale, prefix error / sum)."""
    c = cases()[name]
    o = expected(name)
    nh, nf_pad, nb, _ = c["hists"].shape
    assert out.shape == (nh, 6), out.shape
    worst_g = worst_p = 0.0
    for i, (bg, bf, bb) in enumerate(o["best"]):
        gain, f, b = float(out[i, 0]), out[i, 1], out[i, 2]
        assert f == int(f) and 0 <= f < nf_pad, (name, i, f)
        assert b == int(b) and 0 <= b < nb, (name, i, b)
        if bf is None:
            # the remaining fields are unspecified with no valid split
            assert gain == NEG_INF, (name, i, gain)
            continue
        assert (int(f), int(b)) == (bf, bb), (name, i, (f, b), (bf, bb), gain)
        pre = o["prefix"][i, bf, bb]
        scale = o["scale"][i, bf, bb]
        sums = np.abs(c["hists"][i, bf].astype(np.float64)).sum(axis=0)
        eg = abs(gain - bg) / scale if scale > 0 else abs(gain - bg)
        ep = max(abs(float(out[i, 3]) - pre[0]) / max(sums[0], 1e-300),
                 abs(float(out[i, 4]) - pre[1]) / max(sums[1], 1e-300))
        worst_g, worst_p = max(worst_g, eg), max(worst_p, ep)
        assert eg <= gain_tol, (name, i, "gain", gain, bg, eg, gain_tol)
        assert ep <= prefix_tol, (name, i, "prefix", out[i], pre, ep)
        assert float(out[i, 5]) == pre[2], (name, i, "CL", out[i, 5], pre[2])
    return worst_g, worst_p


def tolerances(name):
    """(gain_tol, prefix_tol) of a case: Family A's gain is within the
    derived 7 * 2^-24 (half of A_MARGIN) and its prefix sums are exact."""
    if cases()[name]["family"] == "A":
        return A_MARGIN / 2, 0.0
    return B_GAIN_BOUND, B_PREFIX_BOUND


# ------------------------------------------------- fixed-point histograms
# scale_g / scale_h for the sibling-scan tests: powers of two, so the int64
# cells hold the float32 values exactly and (cell * (1 / scale)) gives them
# back bit for bit.  "wide" puts the largest |g| cell of a sibling pair's
# parent near 2^60, as the grower's own scale does.
def fixed_scales(name, wide):
    c = cases()[name]
    if not wide:
        return 2.0 ** 44, 2.0 ** 44
    h64 = np.abs(c["hists"].astype(np.float64))
    out = []
    for k in (0, 1):
        top = 2 * max(h64[..., k].max(), 1.0)      # parent = small + big
        out.append(2.0 ** (60 - int(np.ceil(np.log2(top)))))
    return tuple(out)


def fixed_hist(name, hi, scale_g, scale_h):
    """Histogram hi of a case as exact int64 cells (nf_pad, n_bins, 3)."""
    h64 = cases()[name]["hists"][hi].astype(np.float64)
    q = h64 * np.array([scale_g, scale_h, 1.0])
    assert np.all(q == np.round(q)) and np.abs(q).max() < 2.0 ** 61, name
    return torch.from_numpy(q.astype(np.int64))
