"""Float64 oracle and chosen cases for the VW sparse-SGD kernels, shared by
the CPU and GPU test files.  numpy only: nothing here imports the package, so
a mistake shared by the HIP kernel and its float32 torch reference still
shows.

The oracle is a sequential per-example loop written from the update rules.
Every case has index sets that are disjoint across and within examples (the
builders assert it), so the hogwild kernel's result does not depend on
scheduling and must equal the loop up to float32 rounding.
"""
import functools
import itertools
import math

import numpy as np

EPS = 1e-10
F32_EPS = float(np.finfo(np.float32).eps)
LOSSES = ("squared", "logistic", "hinge")


def f32(x):
    """The float32 nearest to x, as a Python float: hyper-parameters reach
    the kernel as floats, so the cases use values that survive the trip."""
    return float(np.float32(x))


LR = f32(0.1)
L2 = f32(0.01)
POWER_TS = (0.5, 0.0, f32(0.3))
# hinge --invariant parks an example exactly on the margin, where the next
# step's y*p < 1 is decided by rounding.  Those cases take their first steps
# with a rate too small to reach the margin and only the last one at LR.
LR_SHORT = f32(1e-4)

# Measured max-norm relative error of the float32 torch reference against
# the oracle on the cases below (worst over every step of every case of the
# family), rounded up.  "exact" = squared or hinge loss with power_t 0.5 or
# 0.0, where every operation is correctly rounded; "transc" = logistic loss
# or power_t 0.3, which go through exp/pow.  The CPU test asserts
# CPU_MARGIN x floor; the GPU test GPU_MARGIN[family] x floor (the fast
# exp/pow intrinsics are a few ulps where libm is under one).  s holds
# copies of |x| and is compared exactly.
#
# Measured: exact w 6.2e-7, g 1.1e-6, preds 1.9e-6; transc w 3.8e-7,
# g 8.8e-7, preds 9.5e-7.  The exact family is the worse one because of
# squared loss on the plain path, where p - y can pass near 0 and the step
# g / sqrt(G + g^2) then amplifies the rounding of p by 1 / sqrt(G); its
# labels are drawn with 4 <= |y| <= 8, away from the starting predictions,
# which keeps that factor (and 32 x floor) small.  The largest preds figure
# is from the squared-loss plain-path edge cases, whose labels are +-1.
FLOOR = {
    "exact": {"w": 7e-7, "g": 1.2e-6, "preds": 2e-6},
    "transc": {"w": 4e-7, "g": 9e-7, "preds": 1e-6},
}
CPU_MARGIN = 4
GPU_MARGIN = {"exact": 4, "transc": 32}
MAX_TOL = 1e-4  # no asserted tolerance may exceed this

# |d - root| <= ROOT_TOL * root for the float32 logistic --invariant solve.
# The solve evaluates e^(q0+d): rounding that sum costs up to
# eps/2 * max(|q0|, d) in the exponent, i.e. that much relative error in the
# exponential term, which moves the root by at most
# eps/2 * max(|q0|, d) * min(1, 1/d) relative (<= 15 eps for |q0| <= 30; the
# q0 > 30 shortcut d = h_eta e^-q0 is off by e^-30).  exp, expm1, the divide
# and the last Newton step add a few eps more.  32 eps covers both.
ROOT_TOL = 32 * F32_EPS
Q0_GRID = (-90.0, -20.0, -8.0, -3.0, -1.0, 0.0, 1.0, 3.0, 10.0, 29.0, 31.0,
           40.0)
H_ETA_GRID = (1e-3, 0.1, 1.0, 5.0, 20.0, 60.0, 300.0)


def family(loss, power_t):
    return "transc" if loss == "logistic" or power_t not in (0.5, 0.0) \
        else "exact"


# ------------------------------------------------------------------ oracle
def dloss(loss, p, y):
    if loss == "squared":
        return p - y
    if loss == "logistic":
        z = y * p
        return -y / (1.0 + math.exp(z)) if z < 700.0 else 0.0
    if loss == "hinge":
        return -y if y * p < 1.0 else 0.0
    raise ValueError(loss)


def logistic_root(q0, h_eta):
    """d >= 0 with e^q0 (e^d - 1) + d = h_eta, by bisection on [0, h_eta]
    until the bracket has no float64 strictly inside it."""
    a = math.exp(q0)

    def f(d):
        return (a * math.expm1(d) if d < 700.0 else math.inf) + d - h_eta

    lo, hi = 0.0, float(h_eta)  # f(lo) <= 0 <= f(hi) throughout
    if hi <= 0.0:
        return 0.0
    while True:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            return lo if -f(lo) <= f(hi) else hi
        if f(mid) > 0.0:
            hi = mid
        else:
            lo = mid


def invariant_move(loss, p, y, h_eta):
    """Exact prediction move of the importance-weight-invariant update."""
    if loss == "squared":
        return (y - p) * -math.expm1(-h_eta)
    if loss == "hinge":
        return y * min(h_eta, max(1.0 - y * p, 0.0))
    if loss == "logistic":
        return y * logistic_root(y * p, h_eta)
    raise ValueError(loss)


def oracle_step(batch, w, g, s, lr, l2, power_t, loss, invariant):
    """One sequential pass over `batch`, updating the float64 tables w, g and
    s (None without --normalized) in place.  Returns (preds, margins) where
    margins[ex] = 1 - y*p, the quantity hinge branches on."""
    n_ex = len(batch.off) - 1
    preds = np.zeros(n_ex)
    val64 = batch.val.astype(np.float64)
    for ex in range(n_ex):
        sl = slice(int(batch.off[ex]), int(batch.off[ex + 1]))
        i = batch.idx[sl]
        x = val64[sl]
        y = float(batch.y[ex])
        h = 1.0 if batch.h is None else float(batch.h[ex])
        p = float(np.sum(w[i] * x))
        preds[ex] = p
        gl = dloss(loss, p, y) * h
        if invariant:
            scale = (g[i] + x * x + EPS) ** (-power_t)
            s_new = None
            if s is not None:
                s_new = np.maximum(s[i], np.abs(x))
                pos = s_new > 0.0
                scale[pos] /= s_new[pos]
            x_norm = float(np.sum(x * x * scale))
            if x_norm <= 0.0:
                continue
            dp = invariant_move(loss, p, y, h * lr * x_norm)
            g_i = gl * x + l2 * w[i]
            w[i] += (dp / x_norm * x - lr * l2 * w[i]) * scale
            g[i] += g_i * g_i
            if s is not None:
                s[i] = s_new
            continue
        if gl == 0.0:
            continue
        g_i = gl * x + l2 * w[i]
        g[i] += g_i * g_i
        scale = (g[i] + EPS) ** (-power_t)
        if s is not None:
            s[i] = np.maximum(s[i], np.abs(x))
            pos = s[i] > 0.0
            scale[pos] /= s[i][pos]
        w[i] -= lr * g_i * scale
    return preds, 1.0 - batch.y.astype(np.float64) * preds


# ------------------------------------------------------------------- cases
class Batch:
    """CSR minibatch: idx int32, val float32, off int64, y float32, h float32
    or None.  Read-only once built."""

    def __init__(self, idx, val, off, y, h):
        self.idx = np.ascontiguousarray(idx, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float32)
        self.off = np.ascontiguousarray(off, dtype=np.int64)
        self.y = np.ascontiguousarray(y, dtype=np.float32)
        self.h = None if h is None else np.ascontiguousarray(
            h, dtype=np.float32)
        assert len(np.unique(self.idx)) == len(self.idx), "indices collide"
        for a in (self.idx, self.val, self.off, self.y, self.h):
            if a is not None:
                a.setflags(write=False)

    @property
    def n_ex(self):
        return len(self.off) - 1

    def touched(self):
        return np.unique(self.idx).astype(np.int64)


def _values(rng, n):
    """|x| in [0.25, 2] with a random sign, float32."""
    return (rng.uniform(0.25, 2.0, n) * rng.choice([-1.0, 1.0], n)).astype(
        np.float32)


def ragged_batch(seed, counts, table, labels="pm1", label_seed=0):
    """Examples with the given feature counts on disjoint slots of a table;
    slot table-1 is always used (by the first entry).  The labels have a
    seed of their own."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    nnz = int(counts.sum())
    assert nnz <= table
    slots = rng.permutation(table - 1)[:max(nnz - 1, 0)]
    idx = np.concatenate([[table - 1], slots])[:nnz]
    off = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=off[1:])
    rng_y = np.random.default_rng([seed, label_seed])
    y = rng_y.choice([-1.0, 1.0], len(counts))
    if labels == "real":
        y = y * rng_y.uniform(4.0, 8.0, len(counts))
    h = rng.uniform(0.25, 4.0, len(counts))
    return Batch(idx, _values(rng, nnz), off, y, h)


def warm_tables(seed, table):
    """w ~ 0.1 N(0,1), g ~ U(0, 0.5) as float32."""
    rng = np.random.default_rng(seed)
    return ((0.1 * rng.normal(size=table)).astype(np.float32),
            rng.uniform(0.0, 0.5, table).astype(np.float32))


def lrs_for(loss, invariant, n_steps):
    if loss == "hinge" and invariant:
        return (LR_SHORT,) * (n_steps - 1) + (LR,)
    return (LR,) * n_steps


def _hinge_invariant_labels(batch, w0):
    """Labels that keep every example either at least 1 inside the margin or
    at least 0.25 beyond it at the start, so that the short-rate steps can
    neither reach nor re-cross it."""
    p0 = np.array([np.sum(w0[batch.idx[a:b]].astype(np.float64)
                          * batch.val[a:b].astype(np.float64))
                   for a, b in zip(batch.off[:-1], batch.off[1:])])
    sign = np.where(p0 >= 0.0, 1.0, -1.0)
    y = np.where(np.abs(p0) >= 1.25, sign, -sign)
    return Batch(batch.idx, batch.val, batch.off, y, batch.h)


class Case:
    """A batch, float32 starting tables, hyper-parameters and the oracle's
    float64 trajectory: steps[k] = (preds, margins, w, g, s) after call k."""

    def __init__(self, name, batch, w0, g0, loss, invariant, power_t,
                 normalized, l2, lrs):
        self.name, self.batch, self.w0, self.g0 = name, batch, w0, g0
        self.loss, self.invariant, self.power_t = loss, invariant, power_t
        self.normalized, self.l2, self.lrs = normalized, l2, lrs
        self.table = len(w0)
        self.family = family(loss, power_t)
        for a in (w0, g0):
            a.setflags(write=False)
        w, g = w0.astype(np.float64), g0.astype(np.float64)
        s = np.zeros(self.table) if normalized else None
        self.steps = []
        for lr in lrs:
            preds, margins = oracle_step(batch, w, g, s, lr, l2, power_t,
                                         loss, invariant)
            snap = (preds, margins, w.copy(), g.copy(),
                    None if s is None else s.copy())
            for a in snap:
                if a is not None:
                    a.setflags(write=False)
            self.steps.append(snap)
        if loss == "hinge":
            # a condition on the inputs, from the oracle alone: no step may
            # depend on which side of y*p < 1 float32 lands
            worst = min(float(np.abs(m).min()) for _, m, *_ in self.steps)
            assert worst >= 1e-3, (name, worst)


GRID_COUNTS = (0, 1, 63, 64, 65, 130, 7, 30)
GRID_TABLE = 1 << 15
GRID_PARAMS = [p for p in itertools.product(
    LOSSES, (False, True), POWER_TS, (False, True), (0.0, L2))]


def grid_id(p):
    loss, inv, pt, norm, l2 = p
    return "%s-%s-pt%.1f-%s-l2_%g" % (loss, "inv" if inv else "plain", pt,
                                      "norm" if norm else "raw", l2)


# the plain hinge update can land an example anywhere, also within 1e-3 of
# the margin; this label draw is one for which no hinge case does (Case
# asserts it)
GRID_LABEL_SEED = 15


@functools.lru_cache(maxsize=None)
def _grid_inputs(labels):
    batch = ragged_batch(11, GRID_COUNTS * 40, GRID_TABLE, labels,
                         GRID_LABEL_SEED)
    w0, g0 = warm_tables(12, GRID_TABLE)
    return batch, w0, g0


@functools.lru_cache(maxsize=None)
def grid_case(loss, invariant, power_t, normalized, l2, n_steps=3):
    batch, w0, g0 = _grid_inputs("real" if loss == "squared" else "pm1")
    if loss == "hinge" and invariant:
        batch = _hinge_invariant_labels(batch, w0)
    return Case(grid_id((loss, invariant, power_t, normalized, l2)), batch,
                w0.copy(), g0.copy(), loss, invariant, power_t, normalized,
                l2, lrs_for(loss, invariant, n_steps))


# edge examples, in order; every one has a nonzero warm w and the case l2 > 0
EDGE_BEYOND, EDGE_H0, EDGE_ZEROS, EDGE_EMPTY, EDGE_PLAIN = range(5)
EDGE_TABLE = 256
EDGE_PARAMS = [p for p in itertools.product(
    LOSSES, (False, True), (0.5, 0.0), (False, True))]


def edge_id(p):
    loss, inv, pt, norm = p
    return "%s-%s-pt%.1f-%s" % (loss, "inv" if inv else "plain", pt,
                                "norm" if norm else "raw")


@functools.lru_cache(maxsize=None)
def edge_case(loss, invariant, power_t, normalized):
    """Five examples on the rules where the kernel and a naive vectorised
    reference part ways: (0) label-side of the margin with y*p = 2, where the
    hinge gradient is zero; (1) importance weight 0; (2) every stored value
    0; (3) no entries; (4) an ordinary example next to them.  Two calls, so
    that the running max of (2) is still 0 when it is divided by again."""
    rng = np.random.default_rng(31)
    counts = [9, 7, 5, 0, 70]
    batch = ragged_batch(32, counts, EDGE_TABLE)
    w0, g0 = warm_tables(33, EDGE_TABLE)
    val, y, h = batch.val.copy(), batch.y.copy(), batch.h.copy()
    off = batch.off
    a, b = off[EDGE_BEYOND], off[EDGE_BEYOND + 1]
    x = val[a:b].astype(np.float64)
    w0[batch.idx[a:b]] = (y[EDGE_BEYOND] * 2.0 * x / np.sum(x * x)).astype(
        np.float32)
    h[EDGE_H0] = 0.0
    val[off[EDGE_ZEROS]:off[EDGE_ZEROS + 1]] = 0.0
    g0[batch.idx[off[EDGE_ZEROS]:off[EDGE_ZEROS + 1]]] = rng.choice(
        [0.0, 0.3], 5).astype(np.float32)
    batch = Batch(batch.idx, val, off, y, h)
    assert np.all(w0[batch.idx] != 0.0)
    if loss == "hinge" and invariant:
        keep = batch.y[EDGE_BEYOND]
        batch = _hinge_invariant_labels(batch, w0)
        assert batch.y[EDGE_BEYOND] == keep
    return Case("edge-" + edge_id((loss, invariant, power_t, normalized)),
                batch, w0, g0, loss, invariant, power_t, normalized, L2,
                lrs_for(loss, invariant, 2))


# launch shapes for the GPU file: name -> (feature counts, table)
SHAPES = {
    "n1": ((65,), 1 << 10),
    "n3": ((130, 0, 1), 1 << 10),
    "n4": ((63, 64, 65, 1), 1 << 10),
    "n5": ((7, 0, 130, 64, 30), 1 << 10),
    "counts": ((0, 1, 63, 64, 65, 130), 1 << 10),
    # one example past 4096 blocks x 4 waves: one wave takes a second trip
    "n16385": ((2,) * 16385, 1 << 16),
}
# one representative configuration per path: (loss, invariant, power_t,
# normalized, l2)
SHAPE_CONFIGS = (("squared", False, 0.5, True, L2),
                 ("logistic", True, 0.5, True, L2))


@functools.lru_cache(maxsize=None)
def shape_case(shape, config):
    counts, table = SHAPES[shape]
    loss, invariant, power_t, normalized, l2 = config
    batch = ragged_batch(41, counts, table,
                         "real" if loss == "squared" else "pm1")
    assert table - 1 in batch.idx
    w0, g0 = warm_tables(42, table)
    return Case("%s-%s" % (shape, grid_id(config)), batch, w0, g0, loss,
                invariant, power_t, normalized, l2, (LR,))


@functools.lru_cache(maxsize=None)
def cancelling_predict_case():
    """A batch and a weight table whose per-example terms w*x alternate in
    sign and nearly cancel: |p| is a small fraction of sum|w*x|."""
    batch = ragged_batch(51, (64, 130, 2, 65, 0, 1), 1 << 10)
    rng = np.random.default_rng(52)
    w = (0.1 * rng.normal(size=1 << 10)).astype(np.float32)
    for a, b in zip(batch.off[:-1], batch.off[1:]):
        k = np.arange(b - a)
        t = np.where(k % 2 == 0, 1.0, -1.0) * (1.0 + 1e-3 * rng.random(b - a))
        w[batch.idx[a:b]] = (t / batch.val[a:b].astype(np.float64)).astype(
            np.float32)
    return batch, w


def predict_oracle(batch, w):
    """(sum w x, sum |w x|) per example in float64."""
    t = w[batch.idx].astype(np.float64) * batch.val.astype(np.float64)
    n = batch.n_ex
    p, pa = np.zeros(n), np.zeros(n)
    for ex in range(n):
        sl = slice(int(batch.off[ex]), int(batch.off[ex + 1]))
        p[ex], pa[ex] = t[sl].sum(), np.abs(t[sl]).sum()
    return p, pa


@functools.lru_cache(maxsize=None)
def root_grid():
    """(q0, h_eta, exact root) over Q0_GRID x H_ETA_GRID, with q0 and h_eta
    rounded to float32 first so that the root is that of the inputs the
    float32 code sees."""
    out = []
    for q0, h_eta in itertools.product(Q0_GRID, H_ETA_GRID):
        q0, h_eta = f32(q0), f32(h_eta)
        out.append((q0, h_eta, logistic_root(q0, h_eta)))
    return tuple(out)


COLLISION_SLOTS, COLLISION_EX, COLLISION_FEATS = 64, 2000, 30
COLLISION_LR = f32(2e-6)


@functools.lru_cache(maxsize=None)
def collision_case():
    """2000 x 30 entries hashed onto 64 slots.  Hinge, plain path,
    power_t 0, no l2, zero w: while no example can reach the margin,
    gl = -y h whatever the interleaving, so w and G are plain sums whose
    only freedom is the order of float additions.  Returns the inputs, the
    float64 sums and, per slot, the sums of absolute terms and entry counts."""
    rng = np.random.default_rng(61)
    nnz = COLLISION_EX * COLLISION_FEATS
    idx = rng.integers(0, COLLISION_SLOTS, nnz).astype(np.int32)
    val = _values(rng, nnz)
    off = np.arange(COLLISION_EX + 1, dtype=np.int64) * COLLISION_FEATS
    y = rng.choice([-1.0, 1.0], COLLISION_EX).astype(np.float32)
    h = rng.uniform(0.25, 4.0, COLLISION_EX).astype(np.float32)
    hx = np.repeat(h.astype(np.float64), COLLISION_FEATS) * val.astype(
        np.float64)
    slot_abs = np.bincount(idx, np.abs(hx), COLLISION_SLOTS)
    # |w_slot| <= lr * sum|h x| at any moment, so |p| < 1 for every example
    assert COLLISION_FEATS * float(np.abs(val).max()) * COLLISION_LR \
        * float(slot_abs.max()) < 1.0
    gl_x = -np.repeat(y.astype(np.float64), COLLISION_FEATS) * hx
    w_terms = -COLLISION_LR * gl_x
    return dict(
        idx=idx, val=val, off=off, y=y, h=h,
        w=np.bincount(idx, w_terms, COLLISION_SLOTS),
        w_abs=np.bincount(idx, np.abs(w_terms), COLLISION_SLOTS),
        g=np.bincount(idx, gl_x * gl_x, COLLISION_SLOTS),
        count=np.bincount(idx, minlength=COLLISION_SLOTS))


def rel_err(got, want):
    """max|got - want| / max|want| in float64 (0/0 counts as 0)."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    num = float(np.abs(got - want).max())
    den = float(np.abs(want).max())
    if not np.isfinite(num):
        return math.inf
    return num / den if den > 0.0 else (0.0 if num == 0.0 else math.inf)
