"""CyberML — anomalous-access detection (core/src/main/python/mmlspark/cyber
parity: anomaly/collaborative_filtering.py AccessAnomaly over ALS,
complement_access.py ComplementAccessTransformer, feature/indexers.py
IdIndexer, feature/scalers.py StandardScalarScaler/LinearScalarScaler).

The ALS factorization runs in torch (normal equations per user/resource —
dense solves batch on the GPU), per-tenant.  Scores are user·resource
affinities; anomalous = low affinity, standardized per tenant so the output
is in z-score units (higher = more anomalous)."""
from __future__ import annotations

from typing import Dict

import numpy as np
import pandas as pd
import torch

from ..core.param import Param, toBool, toFloat, toInt
from ..core.pipeline import Estimator, Model, Transformer
from ..core.registry import register
from ..ops import backend
from ..utils.devices import default_device


@register
class ComplementAccessTransformer(Transformer):
    """Sample (user, resource) pairs NOT present in the access log
    (complement_access.py:148)."""
    tenantCol = Param("tenantCol", "tenant column", "tenant")
    indexedUserCol = Param("indexedUserCol", "user index column", "user_idx")
    indexedResCol = Param("indexedResCol", "resource index column", "res_idx")
    complementsetFactor = Param("complementsetFactor",
                                "complement rows per observed row", 2, toInt)
    seed = Param("seed", "sampling seed", 0, toInt)

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        rng = np.random.default_rng(self.get("seed"))
        tcol, ucol, rcol = (self.get("tenantCol"), self.get("indexedUserCol"),
                            self.get("indexedResCol"))
        out_rows = []
        for tenant, g in df.groupby(tcol, sort=False):
            seen = set(zip(g[ucol], g[rcol]))
            users = g[ucol].unique()
            ress = g[rcol].unique()
            want = len(g) * self.get("complementsetFactor")
            tries = 0
            got = 0
            while got < want and tries < want * 20:
                u = users[rng.integers(0, len(users))]
                r = ress[rng.integers(0, len(ress))]
                tries += 1
                if (u, r) not in seen:
                    seen.add((u, r))
                    out_rows.append({tcol: tenant, ucol: u, rcol: r})
                    got += 1
        return pd.DataFrame(out_rows, columns=[tcol, ucol, rcol])


@register
class IdIndexer(Estimator):
    """Per-tenant contiguous id indexing (feature/indexers.py:136)."""
    inputCol = Param("inputCol", "raw id column", None)
    partitionKey = Param("partitionKey", "tenant column", "tenant")
    outputCol = Param("outputCol", "indexed column", None)
    resetPerPartition = Param("resetPerPartition", "restart ids per tenant",
                              True)

    def _fit(self, df):
        maps: Dict = {}
        if self.get("resetPerPartition"):
            for tenant, g in df.groupby(self.get("partitionKey"), sort=False):
                maps[str(tenant)] = {str(v): i for i, v in
                                     enumerate(pd.unique(g[self.get("inputCol")]))}
        else:
            maps["__all__"] = {str(v): i for i, v in
                               enumerate(pd.unique(df[self.get("inputCol")]))}
        m = IdIndexerModel()
        m.set("idMaps", maps)
        for p in ("inputCol", "partitionKey", "outputCol", "resetPerPartition"):
            m.set(p, self.get(p))
        return m


@register
class IdIndexerModel(Model):
    inputCol = Param("inputCol", "raw id column", None)
    partitionKey = Param("partitionKey", "tenant column", "tenant")
    outputCol = Param("outputCol", "indexed column", None)
    resetPerPartition = Param("resetPerPartition", "restart per tenant", True)
    idMaps = Param("idMaps", "tenant → id map", None, is_complex=True)

    def _transform(self, df):
        maps = self.get("idMaps")
        out = df.copy()
        if self.get("resetPerPartition"):
            out[self.get("outputCol")] = [
                maps.get(str(t), {}).get(str(v), -1)
                for t, v in zip(df[self.get("partitionKey")],
                                df[self.get("inputCol")])]
        else:
            m = maps["__all__"]
            out[self.get("outputCol")] = [m.get(str(v), -1)
                                          for v in df[self.get("inputCol")]]
        return out


@register
class StandardScalarScaler(Estimator):
    """Per-tenant z-score scaler (feature/scalers.py:325)."""
    inputCol = Param("inputCol", "value column", None)
    partitionKey = Param("partitionKey", "tenant column", "tenant")
    outputCol = Param("outputCol", "scaled column", None)
    coefficientFactor = Param("coefficientFactor", "output multiplier", 1.0,
                              toFloat)

    def _fit(self, df):
        stats = {}
        for tenant, g in df.groupby(self.get("partitionKey"), sort=False):
            v = g[self.get("inputCol")].to_numpy(dtype=np.float64)
            stats[str(tenant)] = [float(v.mean()), float(v.std() + 1e-12)]
        m = StandardScalarScalerModel()
        m.set("stats", stats)
        for p in ("inputCol", "partitionKey", "outputCol", "coefficientFactor"):
            m.set(p, self.get(p))
        return m


@register
class StandardScalarScalerModel(Model):
    inputCol = Param("inputCol", "value column", None)
    partitionKey = Param("partitionKey", "tenant column", "tenant")
    outputCol = Param("outputCol", "scaled column", None)
    coefficientFactor = Param("coefficientFactor", "multiplier", 1.0, toFloat)
    stats = Param("stats", "tenant → (mean, std)", None, is_complex=True)

    def _transform(self, df):
        stats = self.get("stats")
        c = self.get("coefficientFactor")
        out = df.copy()
        vals = []
        for t, v in zip(df[self.get("partitionKey")],
                        df[self.get("inputCol")]):
            mu, sd = stats.get(str(t), [0.0, 1.0])
            vals.append(c * (float(v) - mu) / sd)
        out[self.get("outputCol")] = vals
        return out


@register
class LinearScalarScaler(Estimator):
    """Per-tenant min-max → [minRequiredValue, maxRequiredValue]."""
    inputCol = Param("inputCol", "value column", None)
    partitionKey = Param("partitionKey", "tenant column", "tenant")
    outputCol = Param("outputCol", "scaled column", None)
    minRequiredValue = Param("minRequiredValue", "output min", 0.0, toFloat)
    maxRequiredValue = Param("maxRequiredValue", "output max", 1.0, toFloat)

    def _fit(self, df):
        stats = {}
        for tenant, g in df.groupby(self.get("partitionKey"), sort=False):
            v = g[self.get("inputCol")].to_numpy(dtype=np.float64)
            stats[str(tenant)] = [float(v.min()), float(v.max())]
        m = LinearScalarScalerModel()
        m.set("stats", stats)
        for p in ("inputCol", "partitionKey", "outputCol", "minRequiredValue",
                  "maxRequiredValue"):
            m.set(p, self.get(p))
        return m


@register
class LinearScalarScalerModel(Model):
    inputCol = Param("inputCol", "value column", None)
    partitionKey = Param("partitionKey", "tenant column", "tenant")
    outputCol = Param("outputCol", "scaled column", None)
    minRequiredValue = Param("minRequiredValue", "output min", 0.0, toFloat)
    maxRequiredValue = Param("maxRequiredValue", "output max", 1.0, toFloat)
    stats = Param("stats", "tenant → (min, max)", None, is_complex=True)

    def _transform(self, df):
        stats = self.get("stats")
        lo, hi = self.get("minRequiredValue"), self.get("maxRequiredValue")
        out = df.copy()
        vals = []
        for t, v in zip(df[self.get("partitionKey")], df[self.get("inputCol")]):
            mn, mx = stats.get(str(t), [0.0, 1.0])
            scale = (hi - lo) / max(mx - mn, 1e-12)
            vals.append(lo + (float(v) - mn) * scale)
        out[self.get("outputCol")] = vals
        return out


def _als(n_u: int, n_r: int, u_idx, r_idx, ratings, rank=10, reg=0.1,
         iters=10, device="cpu", seed=0):
    """Regularized ALS on sparse triples via batched normal equations."""
    g = torch.Generator().manual_seed(seed)
    U = torch.randn(n_u, rank, generator=g).to(device) * 0.1
    V = torch.randn(n_r, rank, generator=g).to(device) * 0.1
    u = torch.as_tensor(u_idx, dtype=torch.long, device=device)
    r = torch.as_tensor(r_idx, dtype=torch.long, device=device)
    y = torch.as_tensor(ratings, dtype=torch.float32, device=device)
    eye = torch.eye(rank, device=device)

    def solve_side(fix, fix_idx, var_idx, n_var):
        F = fix[fix_idx]  # (nnz, k)
        # per-var Gram matrices and rhs via index_add
        G = torch.zeros(n_var, rank, rank, device=device)
        b = torch.zeros(n_var, rank, device=device)
        G.index_add_(0, var_idx, F.unsqueeze(2) * F.unsqueeze(1))
        b.index_add_(0, var_idx, F * y.unsqueeze(1))
        G = G + reg * eye
        return torch.linalg.solve(G, b)

    for _ in range(iters):
        U = solve_side(V, r, u, n_u)
        V = solve_side(U, u, r, n_r)
    return U, V


def _csr(rows, cols, vals, n_rows, n_cols):
    """(indptr int64, col int32, val float32) of triples, rows ascending and
    columns ascending inside a row, repeated pairs kept in their order."""
    order = torch.argsort(rows * n_cols + cols, stable=True)
    indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n_rows), 0)
    return (indptr, cols[order].to(torch.int32).contiguous(),
            vals[order].contiguous())


def _als_csr(n_u: int, n_r: int, u_idx, r_idx, ratings, rank=10, reg=0.1,
             iters=10, device="cpu", seed=0, implicit=False, alpha=1.0):
    """_als through ops.backend.als_half_step: the user-major and the
    resource-major CSR are built once, every half step forms and solves its
    normal equations per row (als_kernels.hip on a GPU, ops/cpu_ref.py
    elsewhere), and nothing of size nnz x rank x rank exists.  Initial factors
    are _als's: the same draws from the same CPU generator.  Implicit mode
    sums repeated (user, res) pairs first; explicit mode keeps them apart as
    _als does."""
    g = torch.Generator().manual_seed(seed)
    U = torch.randn(n_u, rank, generator=g).to(device) * 0.1
    V = torch.randn(n_r, rank, generator=g).to(device) * 0.1
    u = torch.as_tensor(u_idx, dtype=torch.long, device=device)
    r = torch.as_tensor(r_idx, dtype=torch.long, device=device)
    y = torch.as_tensor(ratings, dtype=torch.float32, device=device)
    if implicit and y.numel():
        # sorted float64 running sums: no atomics, so the same bits every run
        key, order = torch.sort(u * n_r + r, stable=True)
        last = torch.ones_like(key, dtype=torch.bool)
        last[:-1] = key[1:] != key[:-1]
        run = torch.cumsum(y[order].double(), 0)[last]
        y = torch.diff(run, prepend=run.new_zeros(1)).float()
        u, r = key[last] // n_r, key[last] % n_r
    by_user = _csr(u, r, y, n_u, n_r)
    by_res = _csr(r, u, y, n_r, n_u)
    backend.check_als_csr(*by_user, n_r)
    backend.check_als_csr(*by_res, n_u)
    for _ in range(iters):
        U = backend.als_half_step(*by_user, V, reg, alpha, implicit,
                                  check=False)
        V = backend.als_half_step(*by_res, U, reg, alpha, implicit,
                                  check=False)
    return U, V


@register
class AccessAnomaly(Estimator):
    """Collaborative-filtering access-anomaly estimator
    (cyber/anomaly/collaborative_filtering.py AccessAnomaly).

    With the defaults the model is the explicit-feedback torch ALS on the CPU
    that this class has always run.  Any of `device`, `applyImplicitCf`,
    `likelihoodCol`, `lowValue`/`highValue` moves the factorisation to
    ops.backend.als_half_step: per-row normal equations formed and solved in
    one HIP kernel on a GPU (opt out with MMLSPARK_AMD_ALS_FUSED=0), float32
    torch on the CPU.

    `applyImplicitCf=True` is implicit-feedback ALS (Hu, Koren, Volinsky) with
    confidence 1 + alphaParam |r| and preference [r > 0]; no complement set is
    drawn and `complementsetFactor`/`negScore` are ignored.  The reference
    defaults to applyImplicitCf=True; here the default stays False so that
    existing models do not change.

    Differences from the reference that are out of scope: regParam is not
    scaled by a row's interaction count (Spark's count-weighted lambda), there
    is no `nonnegative=True` (NNLS) solve, no `historyAccessDf`, and no
    `separateTenants`/`numBlocks`: tenants are always factorised one by one."""
    tenantCol = Param("tenantCol", "tenant column", "tenant")
    indexedUserCol = Param("indexedUserCol", "user index column", "user_idx")
    indexedResCol = Param("indexedResCol", "resource index column", "res_idx")
    rankParam = Param("rankParam", "ALS rank", 10, toInt)
    regParam = Param("regParam", "ALS regularization", 0.1, toFloat)
    maxIter = Param("maxIter", "ALS iterations", 10, toInt)
    complementsetFactor = Param("complementsetFactor",
                                "negative samples per observed", 2, toInt)
    negScore = Param("negScore", "rating for complement samples", 0.0, toFloat)
    outputCol = Param("outputCol", "anomaly score column", "anomaly_score")
    seed = Param("seed", "seed", 0, toInt)
    device = Param("device", "cpu | cuda | auto: where ALS runs", "cpu")
    applyImplicitCf = Param("applyImplicitCf",
                            "implicit-feedback ALS, no complement sampling",
                            False, toBool)
    alphaParam = Param("alphaParam", "implicit confidence 1 + alpha |r|", 1.0,
                       toFloat)
    likelihoodCol = Param("likelihoodCol",
                          "rating column (None: every row rates 1.0)", None)
    lowValue = Param("lowValue", "ratings are scaled per tenant into "
                     "[lowValue, highValue] when both are set", None)
    highValue = Param("highValue", "upper end of the scaled ratings", None)

    def _ratings(self, df: pd.DataFrame):
        """The per-row ratings the new options ask for, or None for 1.0."""
        lcol = self.get("likelihoodCol")
        lo, hi = self.get("lowValue"), self.get("highValue")
        if (lo is None) != (hi is None):
            raise ValueError("lowValue and highValue must be set together")
        if lcol is None and lo is None:
            return None
        tcol = self.get("tenantCol")
        r = pd.DataFrame({tcol: df[tcol].to_numpy(), "__rating":
                          1.0 if lcol is None else
                          df[lcol].to_numpy(dtype=np.float64)})
        if lo is not None:
            r = LinearScalarScaler(
                inputCol="__rating", partitionKey=tcol, outputCol="__rating",
                minRequiredValue=lo, maxRequiredValue=hi).fit(r).transform(r)
        return r["__rating"].to_numpy(dtype=np.float64)

    def _fit(self, df: pd.DataFrame):
        tcol = self.get("tenantCol")
        ucol, rcol = self.get("indexedUserCol"), self.get("indexedResCol")
        comp = ComplementAccessTransformer(
            tenantCol=tcol, indexedUserCol=ucol, indexedResCol=rcol,
            complementsetFactor=self.get("complementsetFactor"),
            seed=self.get("seed"))
        implicit = self.get("applyImplicitCf")
        rated = self._ratings(df)
        by_rows = (self.get("device") != "cpu" or implicit
                   or rated is not None)
        if rated is not None:
            df = df.assign(__rating=rated)
        factors = {}
        train_scores = []
        for tenant, g in df.groupby(tcol, sort=False):
            if by_rows:
                U, V = self._fit_tenant(g, comp, implicit, rated is not None)
                factors[str(tenant)] = (U.cpu().numpy(), V.cpu().numpy())
                s = (U[torch.as_tensor(g[ucol].to_numpy(), device=U.device)]
                     * V[torch.as_tensor(g[rcol].to_numpy(), device=U.device)]
                     ).sum(dim=1)
                train_scores.append(pd.DataFrame({
                    tcol: tenant, "__raw": (-s).cpu().numpy()}))
                continue
            neg = comp.transform(g)
            n_u = int(g[ucol].max()) + 1
            n_r = int(g[rcol].max()) + 1
            u_idx = np.concatenate([g[ucol].to_numpy(),
                                    neg[ucol].to_numpy()]) if len(neg) \
                else g[ucol].to_numpy()
            r_idx = np.concatenate([g[rcol].to_numpy(),
                                    neg[rcol].to_numpy()]) if len(neg) \
                else g[rcol].to_numpy()
            ratings = np.concatenate([
                np.ones(len(g)),
                np.full(len(neg), self.get("negScore"))]) if len(neg) \
                else np.ones(len(g))
            U, V = _als(n_u, n_r, u_idx, r_idx, ratings,
                        rank=self.get("rankParam"), reg=self.get("regParam"),
                        iters=self.get("maxIter"), seed=self.get("seed"))
            factors[str(tenant)] = (U.cpu().numpy(), V.cpu().numpy())
            s = (U[g[ucol].to_numpy()] * V[g[rcol].to_numpy()]).sum(dim=1)
            train_scores.append(pd.DataFrame({
                tcol: tenant, "__raw": (-s).cpu().numpy()}))
        # per-tenant standardization of the anomaly direction (-affinity)
        scaler = StandardScalarScaler(
            inputCol="__raw", partitionKey=tcol, outputCol="__scaled").fit(
                pd.concat(train_scores, ignore_index=True))
        model = AccessAnomalyModel()
        model.set("userFactors", {k: f[0] for k, f in factors.items()})
        model.set("resFactors", {k: f[1] for k, f in factors.items()})
        model.set("scalerStats", scaler.get("stats"))
        for p in ("tenantCol", "indexedUserCol", "indexedResCol", "outputCol",
                  "device"):
            model.set(p, self.get(p))
        return model

    def _fit_tenant(self, g, comp, implicit, rated):
        """One tenant's factors through _als_csr.  Explicit mode appends the
        complement sample with negScore as _fit does; implicit mode has its
        negatives in Y^T Y and draws none."""
        ucol, rcol = self.get("indexedUserCol"), self.get("indexedResCol")
        u_idx, r_idx = g[ucol].to_numpy(), g[rcol].to_numpy()
        ratings = (g["__rating"].to_numpy(dtype=np.float64) if rated
                   else np.ones(len(g)))
        n_u, n_r = int(u_idx.max()) + 1, int(r_idx.max()) + 1
        if not implicit:
            neg = comp.transform(g)
            if len(neg):
                u_idx = np.concatenate([u_idx, neg[ucol].to_numpy()])
                r_idx = np.concatenate([r_idx, neg[rcol].to_numpy()])
                ratings = np.concatenate([
                    ratings, np.full(len(neg), self.get("negScore"))])
        return _als_csr(n_u, n_r, u_idx.astype(np.int64),
                        r_idx.astype(np.int64), ratings,
                        rank=self.get("rankParam"), reg=self.get("regParam"),
                        iters=self.get("maxIter"),
                        device=default_device(self.get("device")),
                        seed=self.get("seed"), implicit=implicit,
                        alpha=self.get("alphaParam"))


@register
class AccessAnomalyModel(Model):
    tenantCol = Param("tenantCol", "tenant column", "tenant")
    indexedUserCol = Param("indexedUserCol", "user index column", "user_idx")
    indexedResCol = Param("indexedResCol", "resource index column", "res_idx")
    outputCol = Param("outputCol", "anomaly score column", "anomaly_score")
    userFactors = Param("userFactors", "tenant → U", None, is_complex=True)
    resFactors = Param("resFactors", "tenant → V", None, is_complex=True)
    scalerStats = Param("scalerStats", "tenant → (mean,std)", None,
                        is_complex=True)
    device = Param("device", "cpu: per-row loop; cuda | auto: one fused "
                   "launch over the whole frame", "cpu")

    def _tables_on(self, device):
        """The tenants' factor tables laid end to end on `device`, with their
        offsets and scaler statistics: built once per (device, userFactors)
        and kept on the model like the KNN index."""
        uf, vf = self.get("userFactors"), self.get("resFactors")
        key = (str(device), id(uf), id(vf))
        cache = getattr(self, "_table_cache", None)
        if cache is None or cache[0] != key:
            stats = self.get("scalerStats")
            names = [t for t in uf if t in vf]
            st = [stats.get(t, [0.0, 1.0]) for t in names]

            def table(f):
                rows = [np.asarray(f[t], dtype=np.float32) for t in names]
                off = np.cumsum([0] + [len(x) for x in rows], dtype=np.int64)
                return (torch.from_numpy(np.ascontiguousarray(
                    np.concatenate(rows))).to(device),
                    torch.from_numpy(off).to(device))

            U, u_off = table(uf)
            V, v_off = table(vf)
            mean = torch.tensor([s[0] for s in st], dtype=torch.float64)
            std = torch.tensor([s[1] for s in st], dtype=torch.float64)
            cache = (key, {t: i for i, t in enumerate(names)},
                     (U, V, u_off, v_off, mean.to(device), std.to(device)))
            self._table_cache = cache
        return cache[1], cache[2]

    def _transform_fused(self, df: pd.DataFrame, device) -> pd.DataFrame:
        out = df.copy()
        if not self.get("userFactors") or not len(df):
            out[self.get("outputCol")] = np.full(len(df), np.nan)
            return out
        index, (U, V, u_off, v_off, mean, std) = self._tables_on(device)

        def ids(col):      # what the loop rejects becomes -1
            v = pd.to_numeric(df[col], errors="coerce").to_numpy(np.float64)
            ok = (v >= 0) & (v < 2.0 ** 31)
            return torch.from_numpy(
                np.where(ok, v, -1).astype(np.int32)).to(device)

        tenant = np.array([index.get(str(t), -1)
                           for t in df[self.get("tenantCol")]], dtype=np.int32)
        scores = backend.als_score_pairs(
            U, V, ids(self.get("indexedUserCol")),
            ids(self.get("indexedResCol")),
            torch.from_numpy(tenant).to(device), u_off, v_off, mean, std)
        out[self.get("outputCol")] = scores.cpu().numpy().astype(np.float64)
        return out

    def _transform(self, df: pd.DataFrame) -> pd.DataFrame:
        if self.get("device") != "cpu":
            return self._transform_fused(df, default_device(self.get("device")))
        tcol = self.get("tenantCol")
        ucol, rcol = self.get("indexedUserCol"), self.get("indexedResCol")
        uf, vf = self.get("userFactors"), self.get("resFactors")
        stats = self.get("scalerStats")
        scores = []
        for t, u, r in zip(df[tcol], df[ucol], df[rcol]):
            U = uf.get(str(t))
            V = vf.get(str(t))
            if U is None or not (0 <= u < len(U)) or not (0 <= r < len(V)):
                scores.append(float("nan"))
                continue
            raw = -float((U[int(u)] * V[int(r)]).sum())
            mu, sd = stats.get(str(t), [0.0, 1.0])
            scores.append((raw - mu) / sd)
        out = df.copy()
        out[self.get("outputCol")] = scores
        return out
