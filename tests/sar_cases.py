"""Cases and a float64 / int64 numpy oracle for the sparse SAR ops
(ops/hip/sar_kernels.hip, ops/cpu_ref.py, models/sar.py).

The oracle shares no code with what it checks: co-occurrence by explicit
set intersection, similarity values by the same three float32 operations in
numpy (IEEE, so bit-comparable), scores as float64 sums of the float32
inputs, top-k by a lexsort on (-score, item).

Error bound of a device score (float family).  The kernel forms a score as
an fmaf chain from 0.0f over m addends a*s, one rounding per fmaf.  With
u = 2^-24 the computed sum differs from the exact one by at most
((1 + u)^m - 1) * sum|a*s| <= (m + 1) * u * sum|a*s| for every m that occurs
here (m * u << 1); the float64 oracle's own error is 2^-29 times smaller.
The exact family needs no bound: small integer affinities times integer
co-occurrence counts keep every partial sum an integer below 2^24, exact in
float32 under any order."""
import functools

import numpy as np

U24 = 2.0 ** -24
SIMS = ("cooccurrence", "jaccard", "lift")


# ------------------------------------------------------------------ patterns
def csr_of(rows_of_cols, n_cols=None):
    """(indptr int64, col int32) of a list of sorted column lists."""
    indptr = np.zeros(len(rows_of_cols) + 1, np.int64)
    np.cumsum([len(r) for r in rows_of_cols], out=indptr[1:])
    col = (np.concatenate([np.asarray(r, np.int32) for r in rows_of_cols])
           if len(rows_of_cols) and indptr[-1] else np.zeros(0, np.int32))
    return indptr, col.astype(np.int32)


def transpose_pattern(user_items, n_items):
    item_users = [[] for _ in range(n_items)]
    for u, its in enumerate(user_items):
        for i in its:
            item_users[int(i)].append(u)
    return item_users


@functools.lru_cache(maxsize=None)
def cooc_pattern(n_users, n_items):
    """Random holdings.  With 1 or 70 users, user 0 holds every item; with 3
    or 300 users (and more than one item) nobody holds the last item and
    user 0 holds every other one."""
    rng = np.random.default_rng(1000 * n_users + n_items)
    dens = min(0.5, 6.0 / n_items + 0.05)
    user_items = []
    for u in range(n_users):
        if u == 0:
            its = np.arange(n_items)
        else:
            its = np.flatnonzero(rng.random(n_items) < dens)
        if n_items > 1 and n_users in (3, 300):
            its = its[its != n_items - 1]
        user_items.append(tuple(int(x) for x in its))
    return tuple(user_items)


def cooc_counts(user_items, n_items):
    """c[i, j] = number of users holding both, by set intersection."""
    sets = [set(us) for us in transpose_pattern(user_items, n_items)]
    c = np.zeros((n_items, n_items), np.int64)
    for i in range(n_items):
        if not sets[i]:
            continue
        for j in range(i, n_items):
            c[i, j] = c[j, i] = len(sets[i] & sets[j])
    return c


@functools.lru_cache(maxsize=None)
def cooc_counts_of(n_users, n_items):
    return cooc_counts(cooc_pattern(n_users, n_items), n_items)


def similarity_csr(c, threshold, sim):
    """CSR similarity of a count matrix: kept iff c >= max(threshold, 1);
    values by the contract's float32 operations."""
    occ = np.diag(c).copy()
    thr = max(int(threshold), 1)
    indptr = np.zeros(len(c) + 1, np.int64)
    cols, vals = [], []
    for i in range(len(c)):
        j = np.flatnonzero(c[i] >= thr)
        cc = c[i, j]
        v = cc.astype(np.float32)
        if sim == "jaccard":
            v = v / (occ[i] + occ[j] - cc).astype(np.float32)
        elif sim == "lift":
            v = v / (np.float32(occ[i]) * occ[j].astype(np.float32))
        cols.append(j.astype(np.int32))
        vals.append(v.astype(np.float32))
        indptr[i + 1] = indptr[i] + len(j)
    col = np.concatenate(cols) if cols else np.zeros(0, np.int32)
    val = np.concatenate(vals) if vals else np.zeros(0, np.float32)
    return indptr, col.astype(np.int32), val.astype(np.float32)


def densify(indptr, col, val, n_cols, dtype=np.float64):
    out = np.zeros((len(indptr) - 1, n_cols), dtype)
    for r in range(len(indptr) - 1):
        out[r, col[indptr[r]:indptr[r + 1]]] = val[indptr[r]:indptr[r + 1]]
    return out


# -------------------------------------------------------------------- scores
def oracle_scores(aff, sim, n_items):
    """float64 (users, items) scores, sum|a*s| and the number of addends."""
    A = densify(*aff, n_items)
    S = densify(*sim, n_items)
    stored = densify(sim[0], sim[1], np.ones(len(sim[1])), n_items)
    held = densify(aff[0], aff[1], np.ones(len(aff[1])), n_items)
    return A @ S, np.abs(A) @ np.abs(S), held @ stored


def oracle_topk(score, seen, k, remove_seen):
    """(items, scores) of one user: candidates by (-score, item) lexsort,
    padded with (-1, -inf)."""
    items = np.arange(len(score))
    cand = ~seen if remove_seen else np.ones(len(score), bool)
    order = np.lexsort((items, -score))
    order = order[cand[order]][:k]
    out_i = np.full(k, -1, np.int32)
    out_s = np.full(k, -np.inf)
    out_i[:len(order)] = order
    out_s[:len(order)] = score[order]
    return out_i, out_s


def seen_mask(aff, n_items):
    return densify(aff[0], aff[1], (aff[2] > 0).astype(np.float64),
                   n_items) > 0


# --------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def exact_case(n_items):
    """Small integer affinities and co-occurrence counts: every score an
    exact float32 integer.  User 0 has no entries, user 1 one entry, user 2
    every item; user 3's first entry is negative and user 4's second is (the
    value 0 never occurs: zeros are not stored)."""
    n_users = 24
    rng = np.random.default_rng(77 + n_items)
    rows, vals = [], []
    for u in range(n_users):
        if u == 0:
            its = np.zeros(0, np.int64)
        elif u == 1:
            its = np.array([n_items // 2])
        elif u == 2:
            its = np.arange(n_items)
        else:
            m = int(min(n_items, rng.integers(2, 12)))
            its = np.sort(rng.choice(n_items, size=m, replace=False))
        v = rng.integers(1, 4, size=len(its)).astype(np.float32)
        if u == 3:
            v[0] = -2.0
        if u == 4 and len(v) > 1:
            v[1] = -1.0
        rows.append(its)
        vals.append(v)
    indptr, col = csr_of(rows)
    val = np.concatenate(vals).astype(np.float32)
    holdings = [tuple(int(i) for i, x in zip(r, v) if x > 0)
                for r, v in zip(rows, vals)]
    sim = similarity_csr(cooc_counts(holdings, n_items), 1, "cooccurrence")
    return {"aff": (indptr, col, val), "sim": sim, "n_users": n_users,
            "n_items": n_items}


@functools.lru_cache(maxsize=None)
def float_case():
    """300 users x 200 items, about 15 entries per user, random float32
    affinities (one in ten negative), jaccard similarity at threshold 2."""
    n_users, n_items = 300, 200
    rng = np.random.default_rng(5)
    rows, vals = [], []
    for u in range(n_users):
        m = int(rng.integers(10, 21))
        its = np.sort(rng.choice(n_items, size=m, replace=False))
        v = rng.uniform(0.05, 5.0, size=m).astype(np.float32)
        v[rng.random(m) < 0.1] *= np.float32(-1.0)
        rows.append(its)
        vals.append(v)
    indptr, col = csr_of(rows)
    val = np.concatenate(vals).astype(np.float32)
    holdings = [tuple(int(i) for i, x in zip(r, v) if x > 0)
                for r, v in zip(rows, vals)]
    sim = similarity_csr(cooc_counts(holdings, n_items), 2, "jaccard")
    return {"aff": (indptr, col, val), "sim": sim, "n_users": n_users,
            "n_items": n_items}


@functools.lru_cache(maxsize=None)
def case_oracle(kind, n_items=None):
    c = float_case() if kind == "float" else exact_case(n_items)
    score, absum, m = oracle_scores(c["aff"], c["sim"], c["n_items"])
    return {"score": score, "bound": (m + 1) * U24 * absum,
            "seen": seen_mask(c["aff"], c["n_items"])}


def expected_topk(kind, n_items, users, k, remove_seen):
    o = case_oracle(kind, n_items)
    its, scs = [], []
    for u in users:
        i, s = oracle_topk(o["score"][u], o["seen"][u], k, remove_seen)
        its.append(i)
        scs.append(s)
    return np.stack(its), np.stack(scs)


def interactions_frame(aff, with_dups=False, seed=0):
    """A (userIdx, itemIdx, rating) frame whose sparse fit gives `aff`; with
    with_dups every entry is split into two rows that sum to it."""
    import pandas as pd
    indptr, col, val = aff
    u = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    if with_dups:
        half = (val / np.float32(2)).astype(np.float32)
        u = np.concatenate([u, u])
        col = np.concatenate([col, col])
        val = np.concatenate([half, val - half]).astype(np.float32)
    perm = np.random.default_rng(seed).permutation(len(u))
    return pd.DataFrame({"userIdx": u[perm].astype(np.int64),
                         "itemIdx": col[perm].astype(np.int64),
                         "rating": val[perm].astype(np.float32)})


# ------------------------------------------------------------------- running
def to_device(arrays, device):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device)
                 for a in arrays)


def run_cooc(n_users, n_items, threshold, sim, device, tile=0):
    """backend.sar_cooccurrence on the named pattern -> numpy CSR."""
    from mmlspark_amd.ops import backend
    user_items = cooc_pattern(n_users, n_items)
    b = csr_of(user_items)
    bt = csr_of(transpose_pattern(user_items, n_items))
    out = backend.sar_cooccurrence(*to_device(b + bt, device), threshold,
                                   sim, tile=tile)
    assert all(str(t.device).startswith(device) for t in out)
    return tuple(t.cpu().numpy() for t in out)


def check_cooc(got, n_users, n_items, threshold, sim):
    """Bit for bit the oracle's CSR, columns ascending inside every row."""
    want = similarity_csr(cooc_counts_of(n_users, n_items), threshold, sim)
    indptr, col, val = got
    assert indptr.dtype == np.int64 and col.dtype == np.int32 \
        and val.dtype == np.float32
    assert np.array_equal(indptr, want[0])
    assert np.array_equal(col, want[1])
    assert np.array_equal(val.view(np.uint32), want[2].view(np.uint32))
    for r in range(n_items):
        assert (np.diff(col[indptr[r]:indptr[r + 1]]) > 0).all()


def run_recommend(case, users, k, remove_seen, device, tile=0):
    """backend.sar_recommend -> (items, scores) numpy."""
    import torch
    from mmlspark_amd.ops import backend
    ids = None if users is None else torch.tensor(
        list(users), dtype=torch.int32, device=device)
    items, scores = backend.sar_recommend(
        *to_device(case["aff"] + case["sim"], device), ids, k, remove_seen,
        tile=tile)
    assert str(items.device).startswith(device)
    assert items.dtype == torch.int32 and scores.dtype == torch.float32
    return items.cpu().numpy(), scores.cpu().numpy()


def check_exact(items, scores, n_items, users, k, remove_seen):
    want_i, want_s = expected_topk("exact", n_items, users, k, remove_seen)
    assert np.array_equal(items, want_i)
    assert np.array_equal(scores.view(np.uint32),
                          want_s.astype(np.float32).view(np.uint32))


def check_float(items, scores, users, k, remove_seen):
    """The three properties of the float family, for every user."""
    o = case_oracle("float")
    n_items = o["score"].shape[1]
    for r, u in enumerate(users):
        orc, bound, seen = o["score"][u], o["bound"][u], o["seen"][u]
        cand = ~seen if remove_seen else np.ones(n_items, bool)
        got = items[r]
        n_got = min(k, int(cand.sum()))
        assert (got[:n_got] >= 0).all() and (got[n_got:] == -1).all()
        assert np.isneginf(scores[r, n_got:]).all()
        got = got[:n_got]
        assert len(set(got.tolist())) == n_got and cand[got].all()
        sc = scores[r, :n_got].astype(np.float64)
        # 1. every score within its bound of the oracle's score of that item
        assert (np.abs(sc - orc[got]) <= bound[got]).all(), u
        # 2. sorted under (score descending, item ascending)
        assert all(sc[p] > sc[p + 1] or (sc[p] == sc[p + 1]
                                         and got[p] < got[p + 1])
                   for p in range(n_got - 1)), u
        # 3. nothing left out beats the k-th by more than both error bounds
        #    (each of the two device scores is within its own bound)
        if n_got:
            left = cand.copy()
            left[got] = False
            last = got[-1]
            assert (orc[left] <= orc[last] + bound[left] + bound[last]).all(), u
