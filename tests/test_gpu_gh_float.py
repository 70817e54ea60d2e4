"""The arena's float gradient records: `float2 {g, h}` per row in place of the
16-byte fixed-point `{gq, CNT|hq}`, quantised where the histogram loads them
(MMLSPARK_AMD_GROWER_GH_FLOAT, default on).  Nothing may depend on the record
form: the histogram adds the same integers, the scatter moves the records bit
for bit, and every array `grow_tree_native` hands back is the same with the
switch on and off and equals the Python grower's tree.

The histogram's reference record is torch.round(x.double() * scale) (ties to
even, as llrint), packed as the kernel packs it: both forms go through the
`hist_pair_range` binding and every comparison is exact equality of int64."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")

CNT = 1 << 44  # the count bit that rides in the hessian word
N_BINS = 255
N_ARENA = 30_011
# (lo, m): odd lo; one row, under a wave, over a 256-row tile, over one
# unrolled step of a 512-thread block (2048 rows), and 30 000 rows
RANGES = [(37, 1), (37, 63), (37, 257), (37, 2049), (11, 30_000)]
# rows per block: the policy's, one tile (a last block of 1 / 63 / 1 / 1 / 48
# rows), and five tiles (last blocks of 769 and 560 rows: the unrolled loop,
# then the tail loop)
CHUNKS = (0, 256, 1280)
ENV_GH = "MMLSPARK_AMD_GROWER_GH_FLOAT"
ENV_STREAMS = "MMLSPARK_AMD_GROWER_STREAMS"
ENV_NO_NATIVE = "MMLSPARK_AMD_NO_NATIVE_GROWER"


def _scales(g, h, n_global):
    """TreeGrower.set_scales for a session of n_global rows."""
    gmax = max(float(g.abs().max()), 1e-12)
    hmax = max(float(h.max()), 1e-12)
    return (2.0 ** 61) / (n_global * gmax), (2.0 ** 24) / hmax


def _ties(rng, scale, count):
    """float32 values in (0.25, 1) whose float64 product with scale has the
    fraction .5 exactly: the candidates' products are searched, not solved."""
    out = np.zeros(0, dtype=np.float32)
    while out.size < count:
        c = rng.uniform(0.25, 1.0, size=1 << 22).astype(np.float32)
        p = c.astype(np.float64) * scale
        out = np.concatenate([out, c[p - np.floor(p) == 0.5]])
    return out[:count]


@functools.lru_cache(maxsize=None)
def _records(n_global):
    """(g, h) float32 records of the arena, their scales and the reference
    int64 records.  Rows 37.. hold the special values so that every range
    starts on them: a tie first, then +-max, +-0, denormals, more ties."""
    rng = np.random.default_rng(5 + n_global % 1000)
    g = rng.normal(scale=0.3, size=N_ARENA).clip(-0.999, 0.999)
    g = g.astype(np.float32)
    h = rng.uniform(0.0, 0.25, size=N_ARENA).astype(np.float32)
    # max |g| = 1 and max h = 0.25 are planted below, so the scales are known
    # before the ties are searched
    scale_g = (2.0 ** 61) / n_global
    scale_h = (2.0 ** 24) / 0.25
    ties = _ties(rng, scale_g, 16)
    tiny = np.float32(1e-40)  # denormal
    special_g = np.concatenate([
        ties[:1], np.array([1.0, -1.0, 0.0, -0.0, tiny, -tiny,
                            np.float32(1.4e-45)], dtype=np.float32),
        ties[1:8], -ties[8:]])
    assert tiny != 0 and abs(tiny) < np.finfo(np.float32).tiny
    # hessians: 0, the maximum, and ties: scale_h = 2^26, so an odd multiple
    # of 2^-27 lands on .5
    special_h = np.array([3 * 2.0 ** -27, 0.0, 0.25, 0.25, 0.0, 5 * 2.0 ** -27,
                          (2 ** 20 + 1) * 2.0 ** -27, 0.125], dtype=np.float32)
    g[37:37 + special_g.size] = special_g
    h[37:37 + special_h.size] = special_h
    g[N_ARENA - 2:] = [-1.0, ties[0]]
    h[N_ARENA - 2:] = [0.25, 0.0]
    g_t, h_t = torch.from_numpy(g), torch.from_numpy(h)
    assert _scales(g_t, h_t, n_global) == (scale_g, scale_h)
    gq = torch.round(g_t.double() * scale_g).to(torch.int64)
    hq = torch.round(h_t.double() * scale_h).to(torch.int64)
    # the ties are ties, of both signs and in the hessians too
    frac = (g_t.double() * scale_g).frac().abs()
    assert int((frac == 0.5).sum()) >= 17
    assert int(gq.max()) == -int(gq.min()) == round(scale_g) > 2 ** 37
    assert int(((h_t.double() * scale_h).frac() == 0.5).sum()) >= 3
    assert int(hq.max()) == 2 ** 24 and int(hq.min()) == 0
    gh_f = torch.stack([g_t, h_t], dim=1).contiguous()
    gh_q = torch.stack([gq, hq | CNT], dim=1).contiguous()
    return gh_f.cuda(), gh_q.cuda(), scale_g, scale_h


@functools.lru_cache(maxsize=None)
def _planes(nf):
    g = torch.Generator().manual_seed(300 + nf)
    npairs = (nf + 7) // 8
    by = torch.randint(0, N_BINS, (npairs, N_ARENA, 8), generator=g,
                       dtype=torch.uint8)
    base = torch.randint(1, 1000, (npairs * 8, N_BINS, 3), generator=g,
                         dtype=torch.int64)
    return by.view(torch.int64).squeeze(-1).contiguous().cuda(), base.cuda()


@requires_gpu
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("nf", [5, 9, 100])
def test_hist_float_records_equal_int64_records(nf, layout):
    """nf = 5 / 9 / 100: 1 / 2 / 13 planes with 5 / 1 / 4 valid bytes in the
    last one.  Per plane shape and layout: orders 0 / 1, 256 / 512 threads,
    the whole range and both sides of a device left count, five range sizes,
    three rows-per-block settings and the scales of 30 000 and 10^7 rows."""
    from mmlspark_amd.ops import _hip_grower
    npairs = (nf + 7) // 8
    tail = nf - (npairs - 1) * 8
    assert (npairs, tail) == {5: (1, 5), 9: (2, 1), 100: (13, 4)}[nf]
    pair, base = _planes(nf)
    for n_global in (30_000, 10_000_000):
        gh_f, gh_q, scale_g, scale_h = _records(n_global)
        for lo, m in RANGES:
            nl = m // 3
            nl_dev = torch.tensor([nl], dtype=torch.int32, device="cuda")
            for side, rows in ((-1, m), (0, nl), (1, m - nl)):
                for order in (0, 1):
                    for threads in (256, 512):
                        for chunk in CHUNKS:
                            kw = dict(chunk=chunk, threads=threads,
                                      order=order, layout=layout)
                            want = base.clone()
                            _hip_grower.hist_pair_range(
                                pair, gh_q, lo, m, want, N_BINS, tail, nl_dev,
                                side, **kw)
                            got = base.clone()
                            _hip_grower.hist_pair_range(
                                pair, gh_f, lo, m, got, N_BINS, tail, nl_dev,
                                side, scale_g=scale_g, scale_h=scale_h, **kw)
                            tag = (n_global, lo, m, side, order, threads,
                                   chunk)
                            assert torch.equal(got, want), tag
                # the rows were counted, and only into the valid features
                added = got - base
                assert int(added[:nf, :, 2].sum()) == nf * rows, tag
                assert not added[nf:].any(), tag


@requires_gpu
def test_hist_float_records_are_checked():
    from mmlspark_amd.ops import _hip_grower
    pair, base = _planes(5)
    gh_f, _, scale_g, scale_h = _records(30_000)
    hist = base.clone()

    def run(ghq, **kw):
        _hip_grower.hist_pair_range(pair, ghq, 0, 100, hist, N_BINS, 5, **kw)

    with pytest.raises(RuntimeError, match="ghq"):
        run(gh_f[:-1].contiguous())          # size
    with pytest.raises(RuntimeError, match="ghq"):
        run(gh_f.double())                   # dtype
    with pytest.raises(RuntimeError, match="ghq"):
        run(gh_f.t().contiguous().t())       # contiguity
    with pytest.raises(RuntimeError, match="ghq"):
        run(gh_f.cpu())
    with pytest.raises(RuntimeError, match="scales"):
        run(gh_f, scale_g=0.0, scale_h=scale_h)
    torch.cuda.synchronize()
    assert torch.equal(hist, base)


# ------------------------------------------------------------------ scatter
P_ARENA = 20_000
P_RANGES = [(37, 1), (37, 257), (5, 4097), (0, P_ARENA)]
# (chunk, plane_groups): the policy, 1-D grids of many blocks, plane groups
# with a short last group, one plane per group
LAUNCH_SHAPES = [(0, 0), (256, 1), (1024, 2), (4096, 13)]


@functools.lru_cache(maxsize=None)
def _arena(nf):
    """Bin bytes in [1, 250]: thr 0 sends every row right, thr 255 every row
    left.  The records are random bit patterns, NaNs, infinities, -0.0 and
    denormals among them: the scatter must not look inside."""
    g = torch.Generator().manual_seed(500 + nf)
    npairs = (nf + 7) // 8
    by = torch.randint(1, 251, (npairs, P_ARENA, 8), generator=g,
                       dtype=torch.uint8)
    pair = by.view(torch.int64).squeeze(-1).contiguous()
    bits = torch.randint(-2**31, 2**31, (P_ARENA, 2), generator=g,
                         dtype=torch.int64).to(torch.int32)
    bits[0] = torch.tensor([0x7fc00001, -0x80000000])  # NaN payload, -0.0
    bits[1] = torch.tensor([1, 0x7f800000])            # denormal, +inf
    rowid = torch.randperm(P_ARENA, generator=g).to(torch.int32)
    return pair, bits.contiguous(), rowid


def _partition_case(nf, lo, m, feature, thr, cat_words, chunk, groups):
    from mmlspark_amd.ops import _hip_grower
    pair, bits, rowid = _arena(nf)
    src = (pair.cuda(), bits.cuda().view(torch.float32), rowid.cuda())
    assert src[1].dtype == torch.float32 and src[1].shape == (P_ARENA, 2)
    d_pair = torch.full_like(src[0], -99)
    d_gh = torch.full_like(src[1], -7.0)
    d_row = torch.full_like(src[2], -7)
    bins = torch.arange(256)
    if cat_words is None:
        left_of_bin, cat_dev = bins <= thr, None
    else:
        w = torch.from_numpy(cat_words.astype(np.int64))
        left_of_bin = ((w[bins >> 5] >> (bins & 31)) & 1).bool()
        cat_dev = torch.from_numpy(cat_words.view(np.int32)).cuda()
    total = _hip_grower.partition_arena(*src, d_pair, d_gh, d_row, lo, m,
                                        feature, thr, cat_dev, chunk, groups)
    # the CPU's stable partition; outside [lo, lo + m) the fill stays
    seg = slice(lo, lo + m)
    left = left_of_bin[(pair[feature // 8, seg] >> (8 * (feature % 8))) & 0xff]
    order = torch.cat([left.nonzero().flatten(), (~left).nonzero().flatten()])
    e_pair = torch.full_like(pair, -99)
    e_gh = torch.full_like(bits.view(torch.float32), -7.0).view(torch.int32)
    e_row = torch.full_like(rowid, -7)
    e_pair[:, seg] = pair[:, seg][:, order]
    e_gh[seg] = bits[seg][order]
    e_row[seg] = rowid[seg][order]
    tag = (nf, lo, m, feature, thr, chunk, groups)
    assert int(total.item()) == int(left.sum()), tag
    assert torch.equal(d_row.cpu(), e_row), tag
    assert torch.equal(d_gh.view(torch.int32).cpu(), e_gh), tag
    assert torch.equal(d_pair.cpu(), e_pair), tag
    return int(left.sum())


@requires_gpu
@pytest.mark.parametrize("nf", [5, 12, 100])
def test_partition_float_records_matches_cpu_stable_partition(nf):
    for feature in (nf - 1, min(3, nf - 1)):
        for lo, m in P_RANGES:
            for chunk, groups in LAUNCH_SHAPES:
                assert _partition_case(nf, lo, m, feature, 255, None, chunk,
                                       groups) == m   # every row left
                assert _partition_case(nf, lo, m, feature, 0, None, chunk,
                                       groups) == 0   # every row right
                _partition_case(nf, lo, m, feature, 128, None, chunk, groups)
    assert 0 < _partition_case(nf, 0, P_ARENA, nf - 1, 128, None, 0, 0) \
        < P_ARENA


@requires_gpu
def test_partition_float_records_category_bitset():
    words = np.random.default_rng(3).integers(
        0, 2**32, size=8, dtype=np.uint64).astype(np.uint32)
    none, every = np.zeros(8, np.uint32), np.full(8, 0xffffffff, np.uint32)
    for lo, m in P_RANGES:
        for chunk, groups in LAUNCH_SHAPES:
            nl = _partition_case(100, lo, m, 42, 0, words, chunk, groups)
            assert _partition_case(100, lo, m, 42, 0, none, chunk,
                                   groups) == 0
            assert _partition_case(100, lo, m, 42, 0, every, chunk,
                                   groups) == m
    assert 0 < nl < P_ARENA


@requires_gpu
def test_partition_float_records_are_checked():
    from mmlspark_amd.ops import _hip_grower
    pair, bits, rowid = _arena(5)
    pair, rowid = pair.cuda(), rowid.cuda()
    gh = bits.cuda().view(torch.float32)
    dst = (torch.empty_like(pair), torch.empty_like(gh),
           torch.empty_like(rowid))

    def run(src_gh, dst_gh):
        _hip_grower.partition_arena(pair, src_gh, rowid, dst[0], dst_gh,
                                    dst[2], 0, 100, 3, 128)

    with pytest.raises(RuntimeError, match="ghq_src"):
        run(gh[:-1].contiguous(), dst[1])               # size
    with pytest.raises(RuntimeError, match="ghq_src"):
        run(gh.half(), dst[1])                          # dtype
    with pytest.raises(RuntimeError, match="ghq_dst"):
        run(gh, dst[1].t().contiguous().t())            # contiguity
    with pytest.raises(RuntimeError, match="same dtype"):
        run(gh, torch.empty(P_ARENA, 2, dtype=torch.int64, device="cuda"))


# ------------------------------------------------------------------- grower
N_ROWS = 30_000


def _dataset(nf, seed, n_cat=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N_ROWS, nf)).astype(np.float32)
    logit = (X[:, n_cat] * 0.5 + X[:, nf - 1]
             + 0.3 * np.sin(3 * X[:, min(n_cat + 2, nf - 1)]))
    if n_cat:
        cats = rng.integers(0, 24, size=(N_ROWS, n_cat))
        X[:, :n_cat] = cats
        # non-monotone in the category id: needs one-vs-rest set splits
        logit = logit + 1.5 * ((cats[:, 0] % 3 == 0) ^ (cats[:, 1] % 5 == 0))
    y = (logit + 0.3 * rng.normal(size=N_ROWS) > 0.4 * bool(n_cat))
    return X, y.astype(np.float32)


def _clean_env(mp):
    for name in (ENV_GH, ENV_STREAMS, ENV_NO_NATIVE,
                 "MMLSPARK_AMD_FORCE_DIST_GROWER",
                 "MMLSPARK_AMD_GROWER_ROOT_STATIC",
                 "MMLSPARK_AMD_GROWER_ROOT_ONE_WAIT",
                 "MMLSPARK_AMD_GROWER_APPLY"):
        mp.delenv(name, raising=False)


@functools.lru_cache(maxsize=None)
def _grow_inputs(nf, n_cat, num_leaves):
    """One session per case with its first tree's gradients, shared by every
    call and never changed."""
    from mmlspark_amd.models.gbdt.objectives import make_objective
    from mmlspark_amd.models.gbdt.trainer import TrainConfig, TrainingSession
    from mmlspark_amd.parallel.comm import Comm
    X, y = _dataset(nf, seed=170 + nf + n_cat, n_cat=n_cat)
    cfg = TrainConfig(num_iterations=1, num_leaves=num_leaves,
                      min_data_in_leaf=1,
                      categorical_features=list(range(n_cat)) or None)
    ses = TrainingSession(torch.from_numpy(X).cuda(),
                          torch.from_numpy(y).cuda(), cfg,
                          make_objective("binary"), Comm())
    g, h = ses.objective.grad_hess(ses.preds, ses.y, None)
    g, h = g[:, 0].contiguous(), h[:, 0].contiguous()
    ses.grower.set_scales(g, h)
    return ses, g, h


def _grow(nf, n_cat, num_leaves, rows_identity, dist):
    """One direct grow_tree_native call with the arguments
    TreeGrower._grow_native gives it; returns {key: numpy array}."""
    from mmlspark_amd.ops import _hip_grower
    ses, g, h = _grow_inputs(nf, n_cat, num_leaves)
    gr, cfg = ses.grower, ses.cfg
    num_mask = cats_t = None
    if n_cat:
        num_mask = torch.ones(gr.nf_pad, dtype=torch.bool, device="cuda")
        num_mask[:n_cat] = False
        cats_t = torch.arange(n_cat, dtype=torch.int64)
    d = _hip_grower.grow_tree_native(
        gr.binned, gr.binned_pair, ses.all_rows, g, h, cfg.max_bin, gr.nf,
        gr.scale_g, gr.scale_h, cfg.lambda_l1, cfg.lambda_l2,
        float(cfg.min_data_in_leaf), cfg.min_sum_hessian_in_leaf,
        cfg.min_gain_to_split, cfg.max_delta_step, cfg.num_leaves,
        cfg.max_depth, num_mask, cats_t, gr.cat_smooth, None, dist,
        rows_identity=rows_identity)
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in d.items()}


TREE_KEYS = ("feature", "thr_bin", "left", "right", "value", "count", "gain",
             "leaf_index")


def _python_tree(nf, n_cat, num_leaves, mp):
    """The same tree from the Python grower (rows-list kernels): its node
    arrays under grow_tree_native's keys, and each leaf's sorted rows."""
    ses, g, h = _grow_inputs(nf, n_cat, num_leaves)
    mp.setenv(ENV_NO_NATIVE, "1")
    tree, leaves = ses.grower.grow(ses.all_rows, g, h, None)
    mp.delenv(ENV_NO_NATIVE)
    assert leaves is not None, "the Python grower returns its leaves"
    want = {key: getattr(tree, key) for key in TREE_KEYS}
    want["cat_offset"] = tree.cat_offset
    want["cat_words"] = tree.cat_words.view(np.int32)
    rows = {int(lf.node_id): np.sort(lf.rows.cpu().numpy())
            for lf in leaves}
    return want, rows


@requires_gpu
@pytest.mark.parametrize("n_cat", [0, 4])
@pytest.mark.parametrize("num_leaves", [2, 3, 63])
@pytest.mark.parametrize("nf", [5, 9, 100])
def test_grower_same_with_float_and_fixed_records(nf, num_leaves, n_cat,
                                                  monkeypatch):
    _clean_env(monkeypatch)
    want, want_rows = _python_tree(nf, n_cat, num_leaves, monkeypatch)
    for streams in ("1", "3"):
        monkeypatch.setenv(ENV_STREAMS, streams)
        for dist in (False, True):
            for identity in (False, True):
                what = (streams, dist, identity)
                monkeypatch.setenv(ENV_GH, "0")
                off = _grow(nf, n_cat, num_leaves, identity, dist)
                monkeypatch.setenv(ENV_GH, "1")
                on = _grow(nf, n_cat, num_leaves, identity, dist)
                assert on.keys() == off.keys(), what
                for key in off:
                    assert on[key].dtype == off[key].dtype, (what, key)
                    assert np.array_equal(on[key], off[key]), (what, key)
                for key, arr in want.items():
                    assert on[key].dtype == arr.dtype, (what, key)
                    assert np.array_equal(on[key], arr), (what, key)
                offs = on["leaf_offsets"]
                assert len(want_rows) == len(on["leaf_nodes"]), what
                for i, nid in enumerate(on["leaf_nodes"]):
                    assert np.array_equal(
                        np.sort(on["leaf_rows"][offs[i]:offs[i + 1]]),
                        want_rows[int(nid)]), (what, nid)
    assert 3 <= len(on["feature"]) <= 2 * num_leaves - 1
    if n_cat and num_leaves == 63:
        assert (on["cat_offset"] >= 0).any(), "no categorical split was taken"


@requires_gpu
def test_switch_is_validated(monkeypatch):
    _clean_env(monkeypatch)
    for bad in ("2", "on", "-1"):
        monkeypatch.setenv(ENV_GH, bad)
        with pytest.raises(RuntimeError, match=ENV_GH):
            _grow(5, 0, 3, False, False)
