"""Shared cases and float64 oracle of the lambdarank tests (CPU and GPU
files): seeded inputs, the kernel's per-fit tables computed independently of
the code under test, the oracle evaluated once per case, and the per-cell
error bound."""
import functools

import numpy as np
import torch

MIXED_SIZES = [1, 2, 3, 0, 7, 64, 65, 130, 1, 33]
# (sigma, score scale): |x| reaches about 100 at the last one
MIXED_SETTINGS = [(1.0, 3.0), (2.0, 8.0), (1.0, 20.0)]

CASE_NAMES = (["mixed-%g-%g" % st for st in MIXED_SETTINGS]
              + ["one_big", "tiny", "flat", "table", "empty"])


def _case(sizes, score, label, sigma=1.0, label_gain=None):
    return dict(sizes=np.asarray(sizes, dtype=np.int64),
                score=np.asarray(score, dtype=np.float32),
                label=np.asarray(label, dtype=np.float32),
                sigma=float(sigma), label_gain=label_gain)


def mixed(sigma, scale, ties=True):
    """Empty and singleton groups, the wave edge at 64 and 65, a group of
    130 across the 256-thread block edge (documents 143..272); every 7th
    score tied with its neighbour."""
    rng = np.random.default_rng(7)
    n = sum(MIXED_SIZES)
    score = (rng.normal(size=n) * scale).astype(np.float32)
    if ties:
        idx = np.arange(6, n, 7)
        score[idx] = score[idx - 1]
    label = rng.integers(0, 5, size=n)
    return _case(MIXED_SIZES, score, label, sigma)


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case; read-only."""
    if name.startswith("mixed-"):
        _, sigma, scale = name.split("-")
        return mixed(float(sigma), float(scale))
    if name == "mixed_no_ties":
        return mixed(1.0, 3.0, ties=False)
    rng = np.random.default_rng(hash_name(name))
    if name == "one_big":
        n = 1025
        return _case([n], rng.normal(size=n) * 3, rng.integers(0, 5, size=n))
    if name == "tiny":
        sizes = rng.integers(1, 5, size=3000)
        n = int(sizes.sum())
        return _case(sizes, rng.normal(size=n) * 3,
                     rng.integers(0, 5, size=n))
    if name == "flat":
        # group 0: all labels equal; group 1: all scores equal (x == 0 for
        # every pair, ranks decided by index alone)
        score = np.concatenate([rng.normal(size=10) * 3, np.full(12, 0.75)])
        label = np.concatenate([np.full(10, 2), rng.integers(0, 5, size=12)])
        return _case([10, 12], score, label)
    if name == "table":
        # labels 1 and 2 differ while their gains do not: the pair is
        # visited and adds exactly 0
        sizes = [5, 40, 17]
        n = sum(sizes)
        return _case(sizes, rng.normal(size=n) * 3,
                     rng.integers(0, 4, size=n), label_gain=[0, 1, 1, 7])
    if name == "empty":
        return _case([0, 0], [], [])
    raise KeyError(name)


def hash_name(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def gains_of(c):
    y = c["label"]
    if c["label_gain"] is not None:
        return np.asarray(c["label_gain"], dtype=np.float32)[y.astype(int)]
    return (np.float32(2.0) ** y - np.float32(1.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tables(name):
    """The kernel's inputs besides the scores, as numpy arrays, computed
    group by group: offsets i64, gid i32, gain f32, inv_idcg f32 and
    disc_tbl f32 (float64, rounded once); read-only."""
    c = case(name)
    sizes = c["sizes"]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    gid = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    gain = gains_of(c)
    max_m = max(int(sizes.max()) if len(sizes) else 0, 1)
    disc64 = 1.0 / np.log2(np.arange(max_m, dtype=np.float64) + 2.0)
    inv = np.empty(len(sizes), dtype=np.float32)
    for k, (b, e) in enumerate(zip(offsets[:-1], offsets[1:])):
        ideal = np.sort(gain[b:e].astype(np.float64))[::-1]
        inv[k] = 1.0 / max(float((ideal * disc64[:e - b]).sum()), 1e-12)
    return dict(offsets=offsets, gid=gid, gain=gain, inv_idcg=inv,
                disc_tbl=disc64.astype(np.float32))


def op_inputs(name, device="cpu", dtype=torch.float32):
    """Tensors for backend.group_rank / lambdarank_grad on `device`:
    (score, offsets, gid, label, gain, disc_tbl, inv_idcg)."""
    c, t = case(name), tables(name)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return (f(c["score"]).to(dtype), f(t["offsets"]), f(t["gid"]),
            f(c["label"]).to(dtype), f(t["gain"]).to(dtype),
            f(t["disc_tbl"]).to(dtype), f(t["inv_idcg"]).to(dtype))


def stable_ranks(score, offsets):
    """Inverse of np.argsort(-s, kind="stable") per group."""
    rank = np.zeros(score.size, dtype=np.int64)
    for b, e in zip(offsets[:-1], offsets[1:]):
        order = np.argsort(-score[b:e], kind="stable")
        rank[b:e][order] = np.arange(e - b)
    return rank


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Float64 evaluation of the kernel's formulas on the float32 inputs,
    group by group.  Per document: rank, g, h, S_g = sum |t|, S_h = sum of
    the hessian addends (= h), m = group size, X = max |x|; read-only."""
    c, t = case(name), tables(name)
    n = c["score"].size
    sigma = c["sigma"]
    s = c["score"].astype(np.float64)
    y = c["label"]
    gain = t["gain"].astype(np.float64)
    rank = stable_ranks(c["score"], t["offsets"])
    disc = t["disc_tbl"][rank].astype(np.float64) if n else np.zeros(0)
    out = {k: np.zeros(n) for k in ("g", "h", "S_g", "S_h", "m", "X")}
    out["rank"] = rank
    for k, (b, e) in enumerate(zip(t["offsets"][:-1], t["offsets"][1:])):
        out["m"][b:e] = e - b
        if e - b < 2:
            continue
        yi, yj = y[b:e, None], y[None, b:e]
        differ, i_hi = yi != yj, yi > yj
        ds = s[b:e, None] - s[None, b:e]
        x = sigma * np.where(i_hi, ds, -ds)
        ex = np.exp(-np.abs(x))
        q = 1.0 / (1.0 + ex)
        rho = np.where(x < 0, q, ex * q)
        delta = (np.abs(gain[b:e, None] - gain[None, b:e])
                 * np.abs(disc[b:e, None] - disc[None, b:e])
                 * float(t["inv_idcg"][k]))
        tt = np.where(differ, sigma * rho * delta, 0.0)
        hh = np.where(differ, sigma * sigma * (ex * q * q) * delta, 0.0)
        out["g"][b:e] = np.where(i_hi, -tt, tt).sum(axis=1)
        out["S_g"][b:e] = tt.sum(axis=1)
        out["h"][b:e] = hh.sum(axis=1)
        out["S_h"][b:e] = hh.sum(axis=1)
        out["X"][b:e] = np.where(differ, np.abs(x), 0.0).max(axis=1)
    return out


def cell_bound(o, S):
    """|float32 result - oracle| allowed per cell: (m + 12 + X) * 2^-23 * S
    + 1e-37.

    Each addend is a chain of at most 12 correctly rounded or <= 1 ulp
    operations; the rounding of s_hi - s_lo is amplified by |x| through the
    exponential; m - 1 additions follow; denormal results may be flushed."""
    return (o["m"] + 12.0 + o["X"]) * 2.0 ** -23 * S + 1e-37


def check_grads(g, h, name, what=""):
    """Assert both outputs within the bound per cell and exactly 0 where
    S == 0; returns the worst ratio to the bound."""
    o = oracle(name)
    worst = 0.0
    for got, ref, S in ((g, o["g"], o["S_g"]), (h, o["h"], o["S_h"])):
        if got is None:
            continue
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        if not got.size:
            continue
        assert np.isfinite(got).all(), what
        assert (got[S == 0] == 0).all(), f"{what}: non-zero where S == 0"
        ratio = np.abs(got - ref) / cell_bound(o, S)
        i = int(ratio.argmax())
        assert ratio[i] <= 1.0, (what, name, i, got[i], ref[i], ratio[i])
        worst = max(worst, float(ratio[i]))
    return worst


# ---------------------------------------------------------------- NDCG cases
EVAL_AT = [1, 3, 5, 1000]


class _FixedScores:
    """Stands in for a booster in LightGBMRanker._metrics_fn."""

    def __init__(self, scores):
        self.scores = scores

    def predict_raw(self, X):
        return self.scores.unsqueeze(-1)


def host_loop_ndcg(scores, labels, sizes, eval_at, label_gain=None):
    """The per-group numpy loop of LightGBMRanker._metrics_fn on CPU copies
    of the inputs: {k: ndcg@k}."""
    from mmlspark_amd.models.gbdt.estimators import LightGBMRanker
    from mmlspark_amd.parallel.comm import get_comm
    est = LightGBMRanker(evalAt=list(eval_at), labelGain=label_gain)
    fn = est._metrics_fn(torch.as_tensor(np.asarray(sizes, dtype=np.int64)))
    s = torch.as_tensor(scores).detach().cpu().float()
    y = torch.as_tensor(labels).detach().cpu().float()
    # the loop's float64 mean leaves through the [mean, 1] all_reduce tensor,
    # which has the default dtype: float64 here, so nothing is rounded away
    saved = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        out = fn(_FixedScores(s), s, y, None, get_comm())
    finally:
        torch.set_default_dtype(saved)
    return {int(k): out[f"ndcg@{int(k)}"] for k in eval_at}


def recorded_within(recorded, value, bound):
    """A metric recorded by training is the float32 rounding of a float64
    mean (the all_reduce tensor): `recorded` must be the rounding of some
    value within `bound` of `value`.  Rounding is monotone, so that is an
    interval check with no slack added."""
    lo, hi = np.float32(value - bound), np.float32(value + bound)
    return float(lo) <= recorded <= float(hi)


def ndcg_bound(k, n_groups, value):
    """Both sides are float64 and differ only in summation order."""
    return (k + n_groups + 4) * 2.0 ** -52 * abs(value)


@functools.lru_cache(maxsize=None)
def ndcg_case(label_gain=None):
    """(scores, labels, sizes) with empty groups, ties, and a group whose
    gains are all zero; read-only."""
    c = mixed(1.0, 3.0)
    label = c["label"].copy()
    offsets = np.concatenate([[0], np.cumsum(c["sizes"])])
    label[offsets[4]:offsets[5]] = 0  # the group of 7: idcg == 0
    if label_gain is not None:
        label = np.minimum(label, len(label_gain) - 1)
    return c["score"], label, c["sizes"]


def ranker_frame():
    """The data of test_gbdt.test_ranker_validation_ndcg_and_early_stopping:
    120 groups of 20, every fifth group held out."""
    import pandas as pd
    rng = np.random.default_rng(21)
    rows = []
    for gid in range(120):
        q = rng.normal(size=4)
        for _ in range(20):
            x = rng.normal(size=4)
            rel = float(np.clip(round(2 + 1.5 * (q @ x) / 4
                                      + rng.normal() * 0.3), 0, 4))
            rows.append({"features": np.concatenate([q, x]).astype(
                np.float32), "label": rel, "group": gid})
    df = pd.DataFrame(rows)
    df["isVal"] = (df["group"] % 5 == 0)
    return df
