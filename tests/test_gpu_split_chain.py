"""GPU tests for the fused per-split chain of the native GBDT grower: the
count + fused-scatter arena partition, the sibling subtract+scan with the
host arg-max (through whole-model equality with the Python grower, which uses
the rows-list kernels and the device reduce), and the one-kernel prediction
update."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")

N_ARENA = 10_000
RANGES = [(0, 1), (0, 64), (37, 255), (37, 256), (37, 257), (0, 4096),
          (5, 4097), (0, N_ARENA)]
# (chunk, plane_groups): the launcher's own policy, then forced 1-D grids
# with many blocks and a forced plane-group split that leaves a short group
LAUNCH_SHAPES = [(0, 0), (256, 1), (1024, 2)]
SENTINEL = -0x0123456789ABCDEF


def _arena(nf, seed):
    """Random arena on the CPU: bin bytes in [1, 250] so thr=0 sends every
    row right and thr=255 every row left."""
    g = torch.Generator().manual_seed(seed)
    npairs = (nf + 7) // 8
    by = torch.randint(1, 251, (npairs, N_ARENA, 8), generator=g,
                       dtype=torch.uint8)
    pair = by.view(torch.int64).squeeze(-1).contiguous()
    ghq = torch.randint(-2**40, 2**40, (N_ARENA, 2), generator=g,
                        dtype=torch.int64)
    rowid = torch.randperm(N_ARENA, generator=g).to(torch.int32)
    return pair, ghq, rowid


def _expected(pair, ghq, rowid, lo, m, feature, left_of_bin):
    seg = slice(lo, lo + m)
    bv = (pair[feature // 8, seg] >> (8 * (feature % 8))) & 0xff
    left = left_of_bin[bv]
    order = torch.cat([left.nonzero().flatten(), (~left).nonzero().flatten()])
    e_pair = torch.full_like(pair, SENTINEL)
    e_ghq = torch.full_like(ghq, SENTINEL)
    e_row = torch.full_like(rowid, -7)
    e_pair[:, seg] = pair[:, seg][:, order]
    e_ghq[seg] = ghq[seg][order]
    e_row[seg] = rowid[seg][order]
    return e_pair, e_ghq, e_row, int(left.sum())


def _run_case(src_dev, src_cpu, lo, m, feature, thr, cat_words, chunk, groups):
    from mmlspark_amd.ops import _hip_grower
    pair, ghq, rowid = src_cpu
    d_pair = torch.full_like(src_dev[0], SENTINEL)
    d_ghq = torch.full_like(src_dev[1], SENTINEL)
    d_row = torch.full_like(src_dev[2], -7)
    bins = torch.arange(256)
    if cat_words is None:
        left_of_bin = bins <= thr
        bits = None
    else:
        w = torch.from_numpy(cat_words.astype(np.int64))
        left_of_bin = ((w[bins >> 5] >> (bins & 31)) & 1).bool()
        bits = torch.from_numpy(cat_words.view(np.int32)).cuda()
    total = _hip_grower.partition_arena(
        src_dev[0], src_dev[1], src_dev[2], d_pair, d_ghq, d_row, lo, m,
        feature, thr, bits, chunk, groups)
    e_pair, e_ghq, e_row, e_total = _expected(pair, ghq, rowid, lo, m,
                                              feature, left_of_bin)
    tag = (lo, m, feature, thr, chunk, groups)
    assert int(total.item()) == e_total, tag
    assert torch.equal(d_row.cpu(), e_row), tag
    assert torch.equal(d_ghq.cpu(), e_ghq), tag
    assert torch.equal(d_pair.cpu(), e_pair), tag
    return e_total


@requires_gpu
@pytest.mark.parametrize("nf", [5, 12, 100])
def test_arena_partition_matches_cpu_stable_partition(nf):
    """Planes, gh, row ids and the left count equal a stable partition done
    with torch on the CPU; the destination outside [lo, lo+m) keeps its
    sentinel.  nf = 5 / 12 / 100 give 1 / 2 / 13 planes with a short tail."""
    src_cpu = _arena(nf, seed=100 + nf)
    src_dev = tuple(t.cuda() for t in src_cpu)
    # split on the last feature (tail plane) and on one of the first plane
    for feature in (nf - 1, min(3, nf - 1)):
        for lo, m in RANGES:
            for chunk, groups in LAUNCH_SHAPES:
                nl = _run_case(src_dev, src_cpu, lo, m, feature, 255, None,
                               chunk, groups)
                assert nl == m            # every row left
                nl = _run_case(src_dev, src_cpu, lo, m, feature, 0, None,
                               chunk, groups)
                assert nl == 0            # every row right
                _run_case(src_dev, src_cpu, lo, m, feature, 128, None,
                          chunk, groups)  # a mix
    # the mix really is one at the full range
    nl = _run_case(src_dev, src_cpu, 0, N_ARENA, nf - 1, 128, None, 0, 0)
    assert 0 < nl < N_ARENA


@requires_gpu
def test_arena_partition_categorical_bitset():
    """Partition by a 256-bit category set instead of bin <= thr."""
    nf = 100
    src_cpu = _arena(nf, seed=7)
    src_dev = tuple(t.cuda() for t in src_cpu)
    words = np.random.default_rng(3).integers(0, 2**32, size=8,
                                              dtype=np.uint64).astype(np.uint32)
    for lo, m in [(37, 257), (5, 4097), (0, N_ARENA)]:
        for chunk, groups in LAUNCH_SHAPES:
            nl = _run_case(src_dev, src_cpu, lo, m, 42, 0, words, chunk,
                           groups)
    assert 0 < nl < N_ARENA


def _dataset(n, nf, seed, duplicate=False):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, nf)).astype(np.float32)
    if duplicate:
        # two exact copies of the most informative column: their gains tie,
        # so the arg-max over features must take the lower index
        X[:, nf - 2] = X[:, 1]
    y = ((X[:, 0] * 0.5 + X[:, 1] + 0.3 * np.sin(3 * X[:, min(2, nf - 1)])
          + 0.3 * rng.normal(size=n)) > 0).astype(np.float32)
    return X, y


def _fit_strings(X, y, **kw):
    import pandas as pd
    from mmlspark_amd.models.gbdt.estimators import LightGBMClassifier
    df = pd.DataFrame({"features": list(X), "label": y})
    kw = dict(numIterations=10, featureFraction=0.8, device="cuda", **kw)
    m_native = LightGBMClassifier(**kw).fit(df)
    os.environ["MMLSPARK_AMD_NO_NATIVE_GROWER"] = "1"
    try:
        m_py = LightGBMClassifier(**kw).fit(df)
    finally:
        del os.environ["MMLSPARK_AMD_NO_NATIVE_GROWER"]
    return m_native.booster, m_py.booster


@requires_gpu
@pytest.mark.parametrize("nf", [5, 10, 100])
@pytest.mark.parametrize("num_leaves", [31, 63])
@pytest.mark.parametrize("min_data", [1, 20])
def test_native_grower_equals_python_grower(nf, num_leaves, min_data):
    """The native grower (fused chain) and the Python grower (rows-list
    kernels, device reduce, index_add_ update) write the same model string."""
    X, y = _dataset(20_000, nf, seed=nf)
    b_native, b_py = _fit_strings(X, y, numLeaves=num_leaves,
                                  minDataInLeaf=min_data)
    assert max(len(t.feature) for t in b_native.trees) > 3
    assert b_native.save_to_string() == b_py.save_to_string()


@requires_gpu
def test_native_grower_duplicate_columns_tie_break():
    X, y = _dataset(20_000, 10, seed=5, duplicate=True)
    b_native, b_py = _fit_strings(X, y, numLeaves=31, minDataInLeaf=20)
    used = {int(f) for t in b_native.trees for f in t.feature if f >= 0}
    assert 1 in used, used
    assert b_native.save_to_string() == b_py.save_to_string()


@requires_gpu
@pytest.mark.parametrize("nf", [5, 10, 100])
def test_native_grower_equals_python_grower_dist_codepath(nf):
    """Same equality with the device-count path of the distributed grower
    (left count read back from the scatter kernel's block 0)."""
    X, y = _dataset(20_000, nf, seed=11 + nf)
    os.environ["MMLSPARK_AMD_FORCE_DIST_GROWER"] = "1"
    try:
        b_native, b_py = _fit_strings(X, y, numLeaves=63, minDataInLeaf=20)
    finally:
        del os.environ["MMLSPARK_AMD_FORCE_DIST_GROWER"]
    assert b_native.save_to_string() == b_py.save_to_string()


@requires_gpu
def test_apply_leaf_values_equals_index_add():
    """One-kernel prediction update against index_add_ on a strided column:
    7 leaves, one of them empty, 10 000 unique rows."""
    from mmlspark_amd.ops import _hip_grower
    g = torch.Generator().manual_seed(9)
    n = 10_000
    preds = torch.randn(n, 3, generator=g).cuda()
    rows = torch.randperm(n, generator=g).to(torch.int32).cuda()
    sizes = [1500, 1, 0, 2500, 3000, 999, 2000]
    assert sum(sizes) == n
    offsets = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int64)
    values = torch.randn(7, generator=g).cuda()
    expect = preds.clone()
    expanded = torch.repeat_interleave(values, torch.tensor(sizes).cuda())
    expect[:, 1].index_add_(0, rows.long(), expanded)
    _hip_grower.apply_leaf_values(preds[:, 1], rows, offsets, values)
    assert torch.equal(preds, expect)
