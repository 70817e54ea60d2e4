"""GPU tests for the LDS cell layouts of the range-mode arena histogram
(`hist_pair_range`, keyword `layout`):

  0  feature-major, one copy: cell = j * n_bins + b
  1  bin-major, rotated features, one copy: cell = b * 8 + j
  2  bin-major, rotated features, one copy per lane half:
     cell = b * 16 + (lane & 8) + j, the copies added in the flush

In layouts 1 and 2 lane l handles byte (l + t) & 7 of its own word at step t,
so zeroing, row loops, pad-byte predication and flush all differ from layout
0.  The sums are integers: every comparison is exact equality with an int64
oracle computed on the CPU, accumulated into a non-zero base slab.

Deliberate breakages that turn this file red (both built and run against
the 58 binding-level cases):
  * the flush reading only copy 0 of layout 2: 20 cases fail, every layout-2
    case and the environment test, the copy-cancellation test with a
    non-zero g slot;
  * an unrotated byte with the new cell formula (the bin taken from byte t
    of the word while the cell uses j = (l + t) & 7): 33 cases fail, those
    of layouts 1 and 2 in which two features of a plane differ in their
    bins."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")

N_ARENA = 20_000
CNT = 1 << 44  # the count bit that rides in the hessian word
LAYOUTS = [0, 1, 2]
# (lo, m) around one tile (1024 rows) and one unrolled step (4 tiles) of the
# widest block, and the whole arena
RANGES = [(0, 1), (37, 1023), (37, 1024), (37, 1025), (5, 4097),
          (0, N_ARENA)]
ENV_LAYOUT = "MMLSPARK_AMD_HIST_LAYOUT"
ENV_OTHERS = ("MMLSPARK_AMD_HIST_THREADS", "MMLSPARK_AMD_HIST_ORDER")


def _oracle(by, gq, hq, base, nf, a, k):
    """base + exact (g, h, count) sums of rows [a, a + k) for the first nf
    features of the byte planes by (npairs, n, 8)."""
    npairs, n, _ = by.shape
    bins = by.permute(0, 2, 1).reshape(npairs * 8, n)[:nf].long()
    vals = torch.stack([gq, hq, torch.ones(n, dtype=torch.int64)], dim=1)
    out = base.clone()
    for f in range(nf):
        out[f].index_add_(0, bins[f, a:a + k], vals[a:a + k])
    return out


def _subranges(lo, m):
    """(side, nl, a, k): the whole range, and its left / right part for device
    left counts 0, m // 3 and m."""
    out = [(-1, None, lo, m)]
    for nl in sorted({0, m // 3, m}):
        out += [(0, nl, lo, nl), (1, nl, lo + nl, m - nl)]
    return out


@functools.lru_cache(maxsize=None)
def _case(nf, n_bins=255):
    """Arena, base slab and exact histograms for nf features, built once and
    shared by every layout: every byte of every plane is a valid bin, pad
    bytes included, so a kernel that read a pad byte would show."""
    g = torch.Generator().manual_seed(900 + nf)
    npairs = (nf + 7) // 8
    by = torch.randint(0, n_bins, (npairs, N_ARENA, 8), generator=g,
                       dtype=torch.uint8)
    pair = by.view(torch.int64).squeeze(-1).contiguous()
    gq = torch.randint(-2**40, 2**40, (N_ARENA,), generator=g,
                       dtype=torch.int64)
    hq = torch.randint(0, 2**24, (N_ARENA,), generator=g, dtype=torch.int64)
    ghq = torch.stack([gq, hq | CNT], dim=1).contiguous()
    base = torch.randint(1, 1000, (npairs * 8, n_bins, 3), generator=g,
                         dtype=torch.int64)
    expect = {}
    for lo, m in RANGES:
        for _, _, a, k in _subranges(lo, m):
            if (a, k) not in expect:
                expect[(a, k)] = _oracle(by, gq, hq, base, nf, a, k).cuda()
    full = expect[(0, N_ARENA)] - base.cuda()
    assert int(full[:nf, :, 2].sum()) == nf * N_ARENA
    return pair.cuda(), ghq.cuda(), base.cuda(), expect


def _check_ranges(nf, layout, chunks, threads=0, order=-1):
    from mmlspark_amd.ops import _hip_grower
    pair_d, ghq_d, base_d, expect = _case(nf)
    npairs = (nf + 7) // 8
    tail_bytes = nf - (npairs - 1) * 8
    for lo, m in RANGES:
        for side, nl, a, k in _subranges(lo, m):
            nl_dev = (None if nl is None else
                      torch.tensor([nl], dtype=torch.int32, device="cuda"))
            want = expect[(a, k)]
            for chunk in chunks:
                hist = base_d.clone()
                _hip_grower.hist_pair_range(
                    pair_d, ghq_d, lo, m, hist, 255, tail_bytes, nl_dev, side,
                    chunk, threads=threads, order=order, layout=layout)
                tag = (lo, m, side, nl, chunk)
                assert torch.equal(hist[:nf], want[:nf]), tag
                # pad features: nothing added
                assert torch.equal(hist[nf:], base_d[nf:]), tag


@requires_gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("nf", [1, 5, 8, 9, 100])
def test_hist_layouts_plane_shapes_match_int64_oracle(nf, layout):
    """nf = 1 / 5 / 8 / 9 / 100: 1 / 1 / 1 / 2 / 13 planes with 1 / 5 / 8 /
    1 / 4 valid bytes in the last one; the policy's rows per block and one
    tile of the widest block."""
    npairs = (nf + 7) // 8
    assert (npairs, nf - (npairs - 1) * 8) == {
        1: (1, 1), 5: (1, 5), 8: (1, 8), 9: (2, 1), 100: (13, 4)}[nf]
    _check_ranges(nf, layout, chunks=(0, 1024))


@requires_gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_hist_layouts_widths_and_orders(threads, order, layout):
    """Two planes, the second with one valid byte; 1024-row chunks give 20
    chunks over the whole arena, so order 1 launches padding blocks; 5120 is
    one unrolled step of the widest block plus a tile."""
    _check_ranges(9, layout, chunks=(0, 1024, 5120), threads=threads,
                  order=order)


PATTERNS = ["zero", "last", "parity", "run8", "random"]


@functools.lru_cache(maxsize=None)
def _pattern_case(n_bins, pattern):
    """12 features (two planes, four valid bytes in the second) whose bins
    follow one pattern in every byte, pad bytes included."""
    g = torch.Generator().manual_seed(40 + n_bins)
    nf, npairs = 12, 2
    row = torch.arange(N_ARENA)
    if pattern == "zero":
        col = torch.zeros(N_ARENA, dtype=torch.long)
    elif pattern == "last":
        col = torch.full((N_ARENA,), n_bins - 1, dtype=torch.long)
    elif pattern == "parity":
        col = (row & 1).clamp(max=n_bins - 1)
    elif pattern == "run8":
        col = (row // 8) % n_bins
    else:
        col = None
    if col is None:
        by = torch.randint(0, n_bins, (npairs, N_ARENA, 8), generator=g,
                           dtype=torch.int64).to(torch.uint8)
    else:
        by = col.to(torch.uint8)[None, :, None].expand(npairs, N_ARENA, 8)
        by = by.contiguous()
    pair = by.view(torch.int64).squeeze(-1).contiguous()
    gq = torch.randint(-2**40, 2**40, (N_ARENA,), generator=g,
                       dtype=torch.int64)
    hq = torch.randint(0, 2**24, (N_ARENA,), generator=g, dtype=torch.int64)
    ghq = torch.stack([gq, hq | CNT], dim=1).contiguous()
    base = torch.randint(1, 1000, (npairs * 8, n_bins, 3), generator=g,
                         dtype=torch.int64)
    expect = {(a, k): _oracle(by, gq, hq, base, nf, a, k).cuda()
              for a, k in ((0, N_ARENA), (37, 1025))}
    return pair.cuda(), ghq.cuda(), base.cuda(), expect


@requires_gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_bins", [1, 2, 16, 255, 256])
def test_hist_layouts_bin_extremes(n_bins, layout):
    """The first and the last cell of every feature, neighbouring lanes on
    one cell (parity, runs of 8 rows: a whole lane half on one bin) and the
    largest LDS allocation (256 bins)."""
    from mmlspark_amd.ops import _hip_grower
    for pattern in PATTERNS:
        pair_d, ghq_d, base_d, expect = _pattern_case(n_bins, pattern)
        for (a, k), want in expect.items():
            for threads in (256, 1024):
                hist = base_d.clone()
                _hip_grower.hist_pair_range(
                    pair_d, ghq_d, a, k, hist, n_bins, 4, threads=threads,
                    layout=layout)
                tag = (pattern, a, k, threads)
                assert torch.equal(hist[:12], want[:12]), tag
                assert torch.equal(hist[12:], base_d[12:]), tag


@requires_gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bins", ["one", "paired"])
def test_hist_layouts_copies_cancel_in_g(bins, layout):
    """gq = +x in the rows that the low lane half of every 16 lanes reads
    (range and chunks start at multiples of 16, so that is row & 8 == 0) and
    -x eight rows later, with the same bins: every g slot sums to exactly 0
    while each copy of layout 2 holds about +-2^60, and h and count do not
    cancel.  A flush that read one copy, or added them after unpacking the
    wrong plane, cannot pass."""
    from mmlspark_amd.ops import _hip_grower
    m = N_ARENA
    assert m % 16 == 0
    g = torch.Generator().manual_seed(77)
    nf, npairs, n_bins = 12, 2, 255
    row = torch.arange(m)
    low = (row & 8) == 0
    x_max = 2**61 // m
    if bins == "one":
        by = torch.full((npairs, m, 8), 3, dtype=torch.uint8)
        x = torch.full((m,), x_max, dtype=torch.int64)
    else:
        by = torch.randint(0, n_bins, (npairs, m, 8), generator=g,
                           dtype=torch.uint8)
        x = torch.randint(x_max // 2, x_max, (m,), generator=g,
                          dtype=torch.int64)
        # rows r and r + 8 share bins and |x|
        src = row - 8 * (~low).long()
        by = by[:, src].contiguous()
        x = x[src]
    gq = torch.where(low, x, -x)
    hq = torch.randint(1, 2**24, (m,), generator=g, dtype=torch.int64)
    pair = by.view(torch.int64).squeeze(-1).contiguous()
    ghq = torch.stack([gq, hq | CNT], dim=1).contiguous()
    base = torch.randint(1, 1000, (npairs * 8, n_bins, 3), generator=g,
                         dtype=torch.int64)
    want = _oracle(by, gq, hq, base, nf, 0, m)
    assert torch.equal(want[:, :, 0], base[:, :, 0])  # g cancels everywhere
    assert int((want - base)[:nf, :, 2].sum()) == nf * m
    pair_d, ghq_d, base_d, want_d = (t.cuda() for t in (pair, ghq, base, want))
    for threads in (256, 512, 1024):
        for chunk in (0, 4096, m):
            hist = base_d.clone()
            _hip_grower.hist_pair_range(pair_d, ghq_d, 0, m, hist, n_bins, 4,
                                        chunk=chunk, threads=threads,
                                        layout=layout)
            assert torch.equal(hist, want_d), (threads, chunk)


@requires_gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_hist_layouts_packed_cell_bound(layout):
    """One plane, 2^19 rows in one block and one bin with hq = 2^24: the
    packed cnt|h cells of a block sum to h = 2^43 (44 bits) and count = 2^19
    (20 bits) with no carry between the fields, also after the two copies of
    layout 2 are added."""
    from mmlspark_amd.ops import _hip_grower
    m, n_bins, b = 1 << 19, 255, 200
    pair_d = torch.full((1, m, 8), b, dtype=torch.uint8,
                        device="cuda").view(torch.int64).squeeze(-1)
    ghq_d = torch.empty(m, 2, dtype=torch.int64, device="cuda")
    ghq_d[:, 0] = 3
    ghq_d[:, 1] = (1 << 24) | CNT
    base_d = torch.arange(8 * n_bins * 3, dtype=torch.int64,
                          device="cuda").view(8, n_bins, 3) + 1
    want = base_d.clone()
    want[:, b, 0] += 3 * m
    want[:, b, 1] += 1 << 43
    want[:, b, 2] += m
    hist = base_d.clone()
    _hip_grower.hist_pair_range(pair_d.contiguous(), ghq_d, 0, m, hist,
                                n_bins, 8, chunk=m, layout=layout)
    assert torch.equal(hist, want)


@requires_gpu
def test_hist_layout_environment_and_keyword(monkeypatch):
    """The environment is read at every launch; an explicit keyword wins; bad
    values raise and leave the slab alone."""
    from mmlspark_amd.ops import _hip_grower
    for name in ENV_OTHERS:
        monkeypatch.delenv(name, raising=False)
    pair_d, ghq_d, base_d, expect = _case(9)
    want = expect[(0, N_ARENA)]

    def run(**kw):
        hist = base_d.clone()
        _hip_grower.hist_pair_range(pair_d, ghq_d, 0, N_ARENA, hist, 255, 1,
                                    **kw)
        return hist

    monkeypatch.delenv(ENV_LAYOUT, raising=False)
    assert torch.equal(run(), want)
    for good in ("0", "1", "2"):
        monkeypatch.setenv(ENV_LAYOUT, good)
        assert torch.equal(run(), want), good
    for bad in ("3", "-1", "two", "2x"):
        monkeypatch.setenv(ENV_LAYOUT, bad)
        hist = base_d.clone()
        with pytest.raises(RuntimeError, match=ENV_LAYOUT):
            _hip_grower.hist_pair_range(pair_d, ghq_d, 0, N_ARENA, hist, 255,
                                        1)
        assert torch.equal(hist, base_d), bad
        assert torch.equal(run(layout=2), want)
    monkeypatch.delenv(ENV_LAYOUT)
    hist = base_d.clone()
    for layout in (-2, 3, 16):
        with pytest.raises(RuntimeError, match="layout"):
            _hip_grower.hist_pair_range(pair_d, ghq_d, 0, 10, hist, 255, 1,
                                        layout=layout)
    assert torch.equal(hist, base_d)


# ------------------------------------------------------------- grower level
N_ROWS = 20_000
NF = 12


def _dataset(n_cat):
    rng = np.random.default_rng(31 + n_cat)
    X = rng.normal(size=(N_ROWS, NF)).astype(np.float32)
    logit = X[:, n_cat] * 0.5 + X[:, NF - 1] + 0.3 * np.sin(3 * X[:, 4])
    if n_cat:
        cats = rng.integers(0, 24, size=(N_ROWS, n_cat))
        X[:, :n_cat] = cats
        # non-monotone in the category id: needs a one-vs-rest set split
        logit = logit + 1.5 * (cats[:, 0] % 3 == 0)
    y = logit + 0.3 * rng.normal(size=N_ROWS) > 0.4 * bool(n_cat)
    return X, y.astype(np.float32)


def _fit(X, y, monkeypatch, n_cat, layout=None, python_grower=False):
    """Fit once; returns (model string, list of per-tree result dicts)."""
    import pandas as pd
    from mmlspark_amd.models.gbdt.estimators import LightGBMClassifier
    from mmlspark_amd.ops import _hip_grower
    df = pd.DataFrame({"features": list(X), "label": y})
    kw = dict(numIterations=3, numLeaves=15, minDataInLeaf=1, device="cuda")
    if n_cat:
        kw["categoricalSlotIndexes"] = list(range(n_cat))
    grown = []
    real = _hip_grower.grow_tree_native

    def recording(*a, **k):
        d = real(*a, **k)
        grown.append({key: v.cpu().numpy() for key, v in d.items()})
        return d

    with monkeypatch.context() as mp:
        mp.setattr(_hip_grower, "grow_tree_native", recording)
        for name in ENV_OTHERS + (ENV_LAYOUT,):
            mp.delenv(name, raising=False)
        if layout is not None:
            mp.setenv(ENV_LAYOUT, layout)
        if python_grower:
            mp.setenv("MMLSPARK_AMD_NO_NATIVE_GROWER", "1")
        model = LightGBMClassifier(**kw).fit(df)
    return model.booster.save_to_string(), grown


@requires_gpu
@pytest.mark.parametrize("n_cat", [0, 1])
def test_grower_hist_layouts_identical_trees(n_cat, monkeypatch):
    monkeypatch.delenv("MMLSPARK_AMD_FORCE_DIST_GROWER", raising=False)
    X, y = _dataset(n_cat)
    s_py, none = _fit(X, y, monkeypatch, n_cat, python_grower=True)
    assert not none, "the Python grower must not call the native one"
    s_policy, trees_policy = _fit(X, y, monkeypatch, n_cat)
    assert len(trees_policy) == 3
    assert max(len(t["feature"]) for t in trees_policy) == 2 * 15 - 1
    assert s_policy == s_py
    for layout in ("0", "1", "2"):
        s, trees = _fit(X, y, monkeypatch, n_cat, layout=layout)
        assert len(trees) == len(trees_policy), layout
        for t, (got, want) in enumerate(zip(trees, trees_policy)):
            assert got.keys() == want.keys()
            for key in want:
                assert got[key].dtype == want[key].dtype, (layout, t, key)
                assert np.array_equal(got[key], want[key]), (layout, t, key)
        assert s == s_py, layout


@requires_gpu
def test_grower_hist_layout_env_is_validated(monkeypatch):
    """A bad value raises from grow_tree_native before any chain is in
    flight: no tree is returned."""
    X, y = _dataset(0)
    for bad in ("3", "-1", "banked"):
        with pytest.raises(RuntimeError, match=ENV_LAYOUT):
            _fit(X, y, monkeypatch, 0, layout=bad)
