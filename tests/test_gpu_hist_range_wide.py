"""GPU tests for the launch shapes of the range-mode arena histogram
(`hist_pair_range`): block widths of 256, 512 and 1024 threads, the
(chunks, planes) grid and the 1-D order that keeps the planes of a row chunk
on one XCD, and the launcher's own choice of both.

The sums are integers, so every result is compared for equality with an
int64 oracle computed on the CPU, from a non-zero base slab: a chunk that is
missed, or read twice, by any width, order or padding block cannot pass.  The
grower-level test then fits the same model with every forced width and order
and expects the policy's trees and the Python grower's model."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")

N_ARENA = 20_000
N_BINS = 255
CNT = 1 << 44  # the count bit that rides in the hessian word
# ranges (lo, m) around one tile (1024 rows) and one unrolled step (4 tiles)
# of the widest block
RANGES = [(0, 1), (37, 1023), (37, 1024), (37, 1025), (0, 4096), (5, 4097),
          (0, 5121), (0, N_ARENA)]
# the launcher's policy; one tile of the widest block (20 chunks over the
# whole arena: not a multiple of 8, so the 1-D order launches padding blocks,
# and m = 1 launches seven padding groups); one step plus a tile
CHUNKS = [0, 1024, 5120]
ENV_THREADS = "MMLSPARK_AMD_HIST_THREADS"
ENV_ORDER = "MMLSPARK_AMD_HIST_ORDER"


@functools.lru_cache(maxsize=None)
def _case(nf):
    """Arena, base slab and exact histograms for nf features, built once and
    shared by every width: every byte of every plane is a valid bin, pad
    bytes included, so a kernel that read a pad byte would show."""
    g = torch.Generator().manual_seed(700 + nf)
    npairs = (nf + 7) // 8
    by = torch.randint(0, N_BINS, (npairs, N_ARENA, 8), generator=g,
                       dtype=torch.uint8)
    pair = by.view(torch.int64).squeeze(-1).contiguous()
    gq = torch.randint(-2**40, 2**40, (N_ARENA,), generator=g,
                       dtype=torch.int64)
    hq = torch.randint(0, 2**24, (N_ARENA,), generator=g, dtype=torch.int64)
    ghq = torch.stack([gq, hq | CNT], dim=1).contiguous()
    bins = by.permute(0, 2, 1).reshape(npairs * 8, N_ARENA)[:nf].long()
    base = torch.randint(1, 1000, (npairs * 8, N_BINS, 3), generator=g,
                         dtype=torch.int64)
    vals = torch.stack([gq, hq, torch.ones(N_ARENA, dtype=torch.int64)], dim=1)
    expect = {}
    for lo, m in RANGES:
        for nl in sorted({0, m // 3, m}):
            for a, k in ((lo, m), (lo, nl), (lo + nl, m - nl)):
                if (a, k) in expect:
                    continue
                out = base.clone()
                for f in range(nf):
                    out[f].index_add_(0, bins[f, a:a + k], vals[a:a + k])
                expect[(a, k)] = out.cuda()
    full = expect[(0, N_ARENA)] - base.cuda()
    assert int(full[:nf, :, 2].sum()) == nf * N_ARENA
    assert (full[:nf, 0, 2] > 0).all() and (full[:nf, N_BINS - 1, 2] > 0).all()
    return pair.cuda(), ghq.cuda(), base.cuda(), expect


@requires_gpu
@pytest.mark.parametrize("threads", [0, 256, 512, 1024])
@pytest.mark.parametrize("nf", [5, 12, 100])
def test_hist_pair_range_widths_and_orders_match_int64_oracle(nf, threads):
    """nf = 5 / 12 / 100 give 1 / 2 / 13 planes with 5 / 4 / 4 valid bytes in
    the last one.  side = 0 / 1 read the left / right part of the range as
    split by a device count of 0, m // 3 and m."""
    from mmlspark_amd.ops import _hip_grower
    pair_d, ghq_d, base_d, expect = _case(nf)
    npairs = (nf + 7) // 8
    tail_bytes = nf - (npairs - 1) * 8
    assert tail_bytes == {5: 5, 12: 4, 100: 4}[nf]
    for lo, m in RANGES:
        sides = [(-1, None)]
        for nl in sorted({0, m // 3, m}):
            sides += [(0, nl), (1, nl)]
        for side, nl in sides:
            nl_dev = (None if nl is None else
                      torch.tensor([nl], dtype=torch.int32, device="cuda"))
            if side < 0:
                a, k = lo, m
            elif side == 0:
                a, k = lo, nl
            else:
                a, k = lo + nl, m - nl
            want = expect[(a, k)]
            for chunk in CHUNKS:
                for order in (0, 1):
                    hist = base_d.clone()
                    _hip_grower.hist_pair_range(
                        pair_d, ghq_d, lo, m, hist, N_BINS, tail_bytes,
                        nl_dev, side, chunk, threads=threads, order=order)
                    tag = (lo, m, chunk, side, nl, order)
                    assert torch.equal(hist[:nf], want[:nf]), tag
                    # pad features: nothing added
                    assert torch.equal(hist[nf:], base_d[nf:]), tag


@requires_gpu
def test_hist_pair_range_environment_settings(monkeypatch):
    """The environment is read at every launch: good values give the exact
    sums within one process, bad ones raise and leave the slab alone."""
    from mmlspark_amd.ops import _hip_grower
    pair_d, ghq_d, base_d, expect = _case(12)
    want = expect[(0, N_ARENA)]

    def run(**kw):
        hist = base_d.clone()
        _hip_grower.hist_pair_range(pair_d, ghq_d, 0, N_ARENA, hist, N_BINS,
                                    4, **kw)
        return hist

    for threads in ("0", "256", "512", "1024"):
        for order in ("0", "1"):
            monkeypatch.setenv(ENV_THREADS, threads)
            monkeypatch.setenv(ENV_ORDER, order)
            assert torch.equal(run(), want), (threads, order)
    for name, other, bads in ((ENV_THREADS, ENV_ORDER, ("128", "2048", "-1",
                                                         "wide", "512x")),
                              (ENV_ORDER, ENV_THREADS, ("2", "-1", "xcd"))):
        monkeypatch.delenv(other, raising=False)
        for bad in bads:
            monkeypatch.setenv(name, bad)
            hist = base_d.clone()
            with pytest.raises(RuntimeError, match=name):
                _hip_grower.hist_pair_range(pair_d, ghq_d, 0, N_ARENA, hist,
                                            N_BINS, 4)
            assert torch.equal(hist, base_d), (name, bad)
        # an explicit argument wins over the environment, bad or not
        assert torch.equal(run(threads=512, order=1), want)
        monkeypatch.delenv(name)


@requires_gpu
def test_hist_pair_range_rejects_bad_width_and_order(monkeypatch):
    from mmlspark_amd.ops import _hip_grower
    monkeypatch.delenv(ENV_THREADS, raising=False)
    monkeypatch.delenv(ENV_ORDER, raising=False)
    pair_d, ghq_d, base_d, _ = _case(12)
    hist = base_d.clone()
    for threads in (-256, 1, 64, 128, 384, 768, 2048):
        with pytest.raises(RuntimeError, match="threads"):
            _hip_grower.hist_pair_range(pair_d, ghq_d, 0, 10, hist, N_BINS, 4,
                                        threads=threads)
    for order in (-2, 2, 8):
        with pytest.raises(RuntimeError, match="order"):
            _hip_grower.hist_pair_range(pair_d, ghq_d, 0, 10, hist, N_BINS, 4,
                                        order=order)
    assert torch.equal(hist, base_d)


# ------------------------------------------------------------- grower level
N_ROWS = 30_000


def _dataset(nf, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N_ROWS, nf)).astype(np.float32)
    logit = X[:, 0] * 0.5 + X[:, nf - 1] + 0.3 * np.sin(3 * X[:, min(2, nf - 1)])
    y = logit + 0.3 * rng.normal(size=N_ROWS) > 0
    return X, y.astype(np.float32)


def _fit(X, y, monkeypatch, env=None, python_grower=False):
    """Fit once; returns (model string, list of per-tree result dicts)."""
    import pandas as pd
    from mmlspark_amd.models.gbdt.estimators import LightGBMClassifier
    from mmlspark_amd.ops import _hip_grower
    df = pd.DataFrame({"features": list(X), "label": y})
    grown = []
    real = _hip_grower.grow_tree_native

    def recording(*a, **k):
        d = real(*a, **k)
        grown.append({key: v.cpu().numpy() for key, v in d.items()})
        return d

    with monkeypatch.context() as mp:
        mp.setattr(_hip_grower, "grow_tree_native", recording)
        mp.delenv(ENV_THREADS, raising=False)
        mp.delenv(ENV_ORDER, raising=False)
        for name, value in (env or {}).items():
            mp.setenv(name, value)
        if python_grower:
            mp.setenv("MMLSPARK_AMD_NO_NATIVE_GROWER", "1")
        model = LightGBMClassifier(numIterations=4, numLeaves=63,
                                   minDataInLeaf=1, featureFraction=0.8,
                                   device="cuda").fit(df)
    return model.booster.save_to_string(), grown


@requires_gpu
@pytest.mark.parametrize("nf", [5, 100])
def test_grower_hist_widths_and_orders_identical_trees(nf, monkeypatch):
    monkeypatch.delenv("MMLSPARK_AMD_FORCE_DIST_GROWER", raising=False)
    X, y = _dataset(nf, seed=80 + nf)
    s_py, none = _fit(X, y, monkeypatch, python_grower=True)
    assert not none, "the Python grower must not call the native one"
    s_policy, trees_policy = _fit(X, y, monkeypatch)
    assert len(trees_policy) == 4
    assert max(len(t["feature"]) for t in trees_policy) == 2 * 63 - 1
    assert s_policy == s_py
    forced = [{ENV_THREADS: t} for t in ("256", "512", "1024")]
    forced += [{ENV_ORDER: o} for o in ("0", "1")]
    for env in forced:
        s, trees = _fit(X, y, monkeypatch, env=env)
        assert len(trees) == len(trees_policy), env
        for t, (got, want) in enumerate(zip(trees, trees_policy)):
            assert got.keys() == want.keys()
            for key in want:
                assert got[key].dtype == want[key].dtype, (env, t, key)
                assert np.array_equal(got[key], want[key]), (env, t, key)
        assert s == s_py, env


@requires_gpu
def test_grower_hist_env_is_validated(monkeypatch):
    X, y = _dataset(5, seed=2)
    for name, bad in ((ENV_THREADS, "300"), (ENV_THREADS, "many"),
                      (ENV_ORDER, "2")):
        with pytest.raises(RuntimeError, match=name):
            _fit(X, y, monkeypatch, env={name: bad})
