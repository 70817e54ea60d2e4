"""Inputs, float64 reference and checks shared by test_explain_ref.py (CPU)
and test_gpu_explain.py (coalition_values_k on MI355X).

Exact cases: leaf values and base are multiples of 2^-10 in [-1, 1], tree
weights come from {0.5, 1, 1.5, 2}: every term is a multiple of 2^-11, every
partial sum is below 2^5, so float32 sums are exact in any order and the
identity output must equal the reference bit for bit.

Float cases: random float32 leaves, weights and base.  The device starts the
float32 sum at base and adds the n - 1 = t1 - t0 trees by fused multiply-add
(the products are exact), so against the float64 sum of the same n terms
    |raw - raw64| <= g * S,  g = (n-1)u / (1 - (n-1)u),  u = 2^-24,
S the sum of the terms' magnitudes (recursive summation, Higham 4.4).  The
transforms are evaluated in float64 by the device's exp (1 ulp, HIP math API)
and IEEE division; d is the raw bound, a = sigmoid * raw:
  identity  d
  sigmoid   d pushed through the Lipschitz constant: sigmoid * d / 4; plus
            per evaluation 2^-53 |a| / 4 (rounding a), 2^-52 + 2^-53 + 2^-53
            (exp, 1 + e, division; p <= 1) and 2^-53 (1 - p); device and
            reference each evaluate once: 2^-49 * (1 + |a|) covers both
  softmax   every partial derivative is at most 1/4, so sum_k d_k / 4; per
            evaluation x - max (2^-53 |x - max| on the exponent), exp 2^-52,
            the K-term sum (K-1) 2^-53 and the division 2^-53, twice:
            2^-51 * (K + 4 + 2 * spread), spread = max - min of the raw sums
and the float64 mean over B draws adds at most 2 * B * 2^-53 * max|value|."""
import functools

import numpy as np
import pandas as pd
import torch

from mmlspark_amd.explainers.lime import TabularLIME, VectorLIME
from mmlspark_amd.explainers.shap import TabularSHAP, VectorSHAP
from mmlspark_amd.models.gbdt.booster import Booster
from mmlspark_amd.models.gbdt.estimators import (LightGBMClassifier,
                                                 LightGBMRegressionModel,
                                                 LightGBMRegressor)
from mmlspark_amd.models.gbdt.tree import Tree
from mmlspark_amd.ops import backend

LEAVES = (2, 8, 3, 5)      # leaf counts the trees cycle through: 3..15 nodes
TILES = (0, 10, 4)  # 10: several tiles, 15-node tree beyond; 4: most beyond

# name -> nf, nZ, R, per-row masks, B, nb (B == nb and no draws: cycling),
# trees, first tree a single leaf, (t0, t1), K, non-unit weights, categorical
CASES = {
    "nf1-z1-r1-b1-t1": (1, 1, 1, False, 1, 4, 1, False, None, 1, False, False),
    "nf31-z257-r3-rowmasks-b3-t4": (31, 257, 3, True, 3, 7, 4, False, None, 1,
                                    True, False),
    "nf32-z257-r3-cycle5-t5-leaf-first": (32, 257, 3, False, 5, 5, 5, True,
                                          None, 1, False, False),
    "nf33-z1-r3-b3-t9-range": (33, 1, 3, False, 3, 6, 9, True, (2, 7), 1, True,
                               False),
    "nf65-z257-r1-b1-t9-k3-range": (65, 257, 1, True, 1, 9, 9, False, (3, 9),
                                    3, True, False),
    "cat-nan-nf4-z16-r3-cycle5-k3": (4, 16, 3, False, 5, 5, 6, False, None, 3,
                                     False, True),
}


def _tree(rng, n_leaves, nf, exact, cat):
    """Random binary tree as node lists, parents before children."""
    feat, left, right = [-1], [0], [0]
    for _ in range(n_leaves - 1):
        i = int(rng.choice([j for j, f in enumerate(feat) if f < 0]))
        feat[i], left[i], right[i] = int(rng.integers(nf)), len(feat), \
            len(feat) + 1
        feat, left, right = feat + [-1, -1], left + [0, 0], right + [0, 0]
    n = len(feat)
    val = (rng.integers(-1024, 1025, n) / 1024.0 if exact
           else rng.normal(size=n)).astype(np.float32)
    thr = rng.normal(size=n).astype(np.float32)
    is_cat = np.array([cat and f == 0 for f in feat])
    return feat, thr, left, right, val, is_cat


@functools.lru_cache(maxsize=None)
def case(name, exact):  # CPU tensors, as backend.coalition_values takes them
    nf, nZ, R, rowm, B, nb, T, leaf0, rng_t, K, wts, cat = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 17 * exact)
    parts = [_tree(rng, 1 if (leaf0 and t == 0) else LEAVES[t % 4], nf, exact,
                   cat) for t in range(T)]
    cols = [np.concatenate([np.asarray(p[i]) for p in parts]) for i in range(6)]
    is_cat = cols[5]
    cat_off = np.where(is_cat, np.cumsum(is_cat) - 1, -1).astype(np.int32)
    words = rng.integers(0, 2 ** 32, size=8 * int(is_cat.sum()),
                         dtype=np.uint64).astype(np.uint32).view(np.int32)
    offsets = np.cumsum([0] + [len(p[0]) for p in parts]).astype(np.int64)
    if exact:
        w = rng.choice([0.5, 1.0, 1.5, 2.0], T) if wts else np.ones(T)
        base = rng.integers(-1024, 1025, K) / 1024.0
    else:
        w = rng.uniform(0.5, 2.0, T) if wts else np.ones(T)
        base = rng.normal(size=K)
    X = rng.normal(size=(R, nf)).astype(np.float32)
    bg = rng.normal(size=(nb, nf)).astype(np.float32)
    if cat:   # feature 0: the category edges; NaN on either side of a bit
        X[:, 0] = (0.0, 255.0, np.nan)
        bg[:, 0] = (256.0, -1.0, 7.0, np.nan, 3.5)
        X[0, 1] = bg[1, 2] = np.nan
        states = (np.arange(16)[:, None] >> np.arange(4)) & 1   # every mask
        states = states[None].astype(bool)
    else:
        states = rng.random((R if rowm else 1, nZ, nf)) < 0.5
    Wd = (nf + 31) // 32
    packed = np.zeros(states.shape[:2] + (Wd * 4,), np.uint8)
    bits = np.packbits(states, axis=-1, bitorder="little")
    packed[..., :bits.shape[-1]] = bits
    bidx = None if B == nb else rng.integers(0, nb, (R, nZ, B)).astype(np.int32)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt))
    return dict(
        forest=[t(cols[0], np.int32), t(cols[1], np.float32),
                t(cols[2], np.int32), t(cols[3], np.int32),
                t(cols[4], np.float32), t(offsets, np.int64),
                t(w, np.float32)],
        cat_offset=t(cat_off, np.int32) if cat else None,
        cat_words=t(words, np.int32) if cat else None,
        X=t(X, np.float32), bg=t(bg, np.float32), states=states,
        masks=t(packed.view("<i4"), np.int32),
        bidx=None if bidx is None else t(bidx, np.int32), B=B,
        base=t(base, np.float32), K=K, range=rng_t or (0, T))


def run(name, device, exact, transform="identity", classes=None, tile_nodes=0):
    c = case(name, exact)
    dev = lambda v: None if v is None else v.to(device)
    t0, t1 = c["range"]
    if classes is None:
        classes = (1, 0) if transform == "sigmoid" else tuple(range(c["K"]))
    return backend.coalition_values(
        *[dev(a) for a in c["forest"]], dev(c["X"]), dev(c["bg"]),
        dev(c["masks"]), c["bidx"], c["B"], dev(c["base"]), c["K"], transform,
        0.75, classes, start_tree=t0, num_iteration=(t1 - t0) // c["K"],
        cat_offset=dev(c["cat_offset"]), cat_words=dev(c["cat_words"]),
        tile_nodes=tile_nodes)


@functools.lru_cache(maxsize=None)
def reference(name, exact, transform="identity"):
    """(values, bound), (R, nZ, C) float64: samples by float32 select, walked
    node by node under go_left_node's rules; float64(weight) * float64(value)
    summed with base, transformed and averaged in float64; bound as above."""
    c = case(name, exact)
    feat, thr, left, right, val, offsets, w = [a.numpy() for a in c["forest"]]
    X, bg, K, B = c["X"].numpy(), c["bg"].numpy(), c["K"], c["B"]
    R, nZ, (t0, t1) = X.shape[0], c["states"].shape[1], c["range"]
    rows = (np.broadcast_to(np.arange(B), (R, nZ, B)) if c["bidx"] is None
            else c["bidx"].numpy())
    on = np.broadcast_to(c["states"], (R,) + c["states"].shape[1:])
    S = np.where(on[:, :, None, :], X[:, None, None, :], bg[rows])
    S = S.reshape(-1, X.shape[1])                     # (R * nZ * B, nf)
    raw = np.tile(c["base"].numpy().astype(np.float64), (len(S), 1))
    mag = np.abs(raw)
    every = np.arange(len(S))
    for t in range(t0, t1):
        node = np.full(len(S), offsets[t])
        while (feat[node] >= 0).any():
            live = feat[node] >= 0
            xv = S[every, np.maximum(feat[node], 0)]
            go = (xv <= thr[node]) | np.isnan(xv)
            if c["cat_offset"] is not None:
                off = c["cat_offset"].numpy()[node]
                out = np.isnan(xv) | (xv < 0) | (xv >= 256)
                b = np.minimum(np.rint(np.where(out, 0, xv)), 255).astype(np.int64)
                word = c["cat_words"].numpy().view(np.uint32)[
                    np.maximum(off, 0) * 8 + (b >> 5)]
                go = np.where(off >= 0, out | (((word >> (b & 31)) & 1) == 1), go)
            step = offsets[t] + np.where(go, left[node], right[node])
            node = np.where(live, step, node)
        term = np.float64(w[t]) * val[node].astype(np.float64)
        raw[:, t % K] += term
        mag[:, t % K] += np.abs(term)
    n = t1 - t0 + 1
    d = (n - 1) * 2.0 ** -24 / (1 - (n - 1) * 2.0 ** -24) * mag
    if transform == "sigmoid":
        a = 0.75 * raw[:, 0]
        p = 1.0 / (1.0 + np.exp(-a))
        vals = np.stack([p, 1.0 - p], axis=1)         # classes (1, 0)
        d = np.repeat(0.75 * d / 4 + 2.0 ** -49 * (1 + np.abs(a))[:, None], 2, 1)
    elif transform == "softmax":
        e = np.exp(raw - raw.max(axis=1, keepdims=True))
        vals = e / e.sum(axis=1, keepdims=True)
        spread = raw.max(axis=1) - raw.min(axis=1)
        d = np.repeat((d.sum(axis=1) / 4
                       + 2.0 ** -51 * (K + 4 + 2 * spread))[:, None], K, 1)
    else:
        vals = raw
    vals, d = (a.reshape(R, nZ, B, -1) for a in (vals, d))
    bound = d.sum(axis=2) / B + 2 * B * 2.0 ** -53 * np.abs(vals).max(axis=2)
    return vals.sum(axis=2) / B, bound


def worst_share(out, name, transform):
    """Largest |out - reference| / bound of a float case; asserts <= 1."""
    want, bound = reference(name, False, transform)
    share = float((np.abs(out.cpu().numpy() - want) / bound).max())
    assert share <= 1.0, (name, transform, share)
    return share


def trained(device, binary):
    """(model, frame, columns): a small binary classifier, or a regressor made
    exactly summable (shrinkage folded in, leaves and base rounded to 2^-10)."""
    rng = np.random.default_rng(5)
    X = rng.normal(size=(200, 6)).astype(np.float32)
    y = X[:, 0] * X[:, 1] + X[:, 2] + 0.1 * rng.normal(size=200)
    cols = [f"c{i}" for i in range(6)]
    df = pd.DataFrame(X, columns=cols)
    df["features"] = list(X)
    df["label"] = ((y > 0) if binary else y).astype(np.float32)
    kw = dict(featureCols=cols, numIterations=5, numLeaves=7, minDataInLeaf=5,
              device=device)
    if binary:
        return LightGBMClassifier(**kw).fit(df), df, cols
    model = LightGBMRegressor(**kw).fit(df)
    b = model.booster
    for t in b.trees:
        t.value = np.round(t.value * t.shrinkage * 1024) / 1024
        t.shrinkage = 1.0
    b.base_score = (np.round(b.base_score * 1024) / 1024).astype(np.float32)
    b.invalidate_cache()
    return model, df, cols


def spy(monkeypatch):  # the bg argument of every coalition_values call
    seen, real = [], backend.coalition_values
    monkeypatch.setattr(backend, "coalition_values",
                        lambda *a, **kw: seen.append(a[8]) or real(*a, **kw))
    return seen


def check_explainers(device, monkeypatch):
    """fusedSampling on equals off, bit for bit; SHAP with a sampled (B = 1)
    and a cycled background (B = nb = 8).  Three rows in chunks of two: two
    kernel calls per transform, on the one background tensor it uploaded."""
    model, df, cols = trained(device, False)
    cols = dict(inputCols=cols)
    seen = spy(monkeypatch)
    for cls, kw, n, nb in ((TabularSHAP, cols, 100, 40), (VectorSHAP, {}, 100, 40),
                           (TabularSHAP, cols, 600, 8), (VectorSHAP, {}, 600, 8),
                           (TabularLIME, cols, 50, 40), (VectorLIME, {}, 50, 40)):
        off, on = (np.stack(cls(
            model=model, targetCol="prediction", seed=3, rowBatch=2,
            numSamples=n, backgroundData=df.head(nb), fusedSampling=f, **kw
        ).transform(df.iloc[40:43])["explanation"].to_numpy())
            for f in (False, True))
        assert np.array_equal(off, on), (cls.__name__, n)
        first, second = seen[-2:]
        assert first is second and first.device.type == device
    assert len(seen) == 12 and len({id(t) for t in seen}) == 6


def check_fallbacks(device, monkeypatch):
    """No kernel call, and on equals off: a classifier's thresholded prediction
    column; a hand-built stump of a model one feature past the limit."""
    model, df, cols = trained(device, True)
    nf = backend.EXPLAIN_MAX_FEATURES + 1
    stump = Tree([nf - 1, -1, -1], [0.0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 0, 0],
                 [0.0, -1.0, 1.0], [2, 1, 1], [1, 0, 0], [-1, 0, 1])
    wide = LightGBMRegressionModel(
        booster=Booster([stump], "regression", 1, np.zeros(1), nf),
        device=device)
    wdf = pd.DataFrame({"features": list(
        np.random.default_rng(7).normal(size=(4, nf)).astype(np.float32))})
    runs = {
        "prediction": lambda f: TabularSHAP(
            inputCols=cols, model=model, targetCol="prediction", numSamples=40,
            backgroundData=df.head(10), fusedSampling=f).transform(df.tail(2)),
        "too-wide": lambda f: VectorLIME(
            model=wide, targetCol="prediction", numSamples=10,
            backgroundData=wdf.head(3), fusedSampling=f).transform(wdf.tail(1)),
    }
    seen = spy(monkeypatch)
    for name, go in runs.items():
        off, on = (np.stack(go(f)["explanation"].to_numpy())
                   for f in (False, True))
        assert np.array_equal(off, on), name
    assert not seen


def check_binary_additivity(device, monkeypatch):
    """Fused TabularSHAP of a binary probability: base + contributions = p."""
    model, df, cols = trained(device, True)
    seen, rows = spy(monkeypatch), df.head(4)
    out = TabularSHAP(inputCols=cols, model=model, targetCol="probability",
                      targetClasses=[1], numSamples=80, fusedSampling=True,
                      backgroundData=df.head(50)).transform(rows)
    exp = np.stack(out["explanation"].to_numpy())
    probs = np.stack(model.transform(rows)["probability"].to_numpy())[:, 1]
    assert len(seen) == 1
    np.testing.assert_allclose(exp[:, 0, :].sum(axis=1), probs, atol=1e-3)


CHECKS = (check_explainers, check_fallbacks, check_binary_additivity)
