"""Shared ALS cases: CSR builders and a numpy float64 oracle that forms A_u
and b_u densely from the definitions and calls np.linalg.solve."""
import numpy as np
import torch

from .test_cyber import _access_log

U32 = 2.0 ** -24      # unit roundoff of float32


def csr(degrees, n_cols, seed, implicit):
    """Random CSR rows of the given degrees: columns drawn with replacement
    (so they repeat), row 2's first two columns forced equal; implicit
    ratings include negatives and exact zeros."""
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    col = rng.integers(0, n_cols, indptr[-1]).astype(np.int32)
    if len(degrees) > 2 and degrees[2] >= 2:
        col[indptr[2] + 1] = col[indptr[2]]
    val = rng.normal(1.0, 1.0, indptr[-1]).astype(np.float32)
    if implicit:
        val[::5] = 0.0
    return (torch.from_numpy(indptr), torch.from_numpy(col),
            torch.from_numpy(val))


def factors(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, k, generator=g)


def systems(indptr, col, val, Y, reg, alpha, implicit):
    """(A (rows, k, k), b (rows, k)) in float64 from the float32 inputs."""
    indptr, col = indptr.cpu().numpy(), col.cpu().numpy()
    val, Y = val.cpu().numpy().astype(np.float64), Y.cpu().numpy().astype(np.float64)
    n, k = len(indptr) - 1, Y.shape[1]
    A = np.zeros((n, k, k))
    b = np.zeros((n, k))
    G = Y.T @ Y
    for u in range(n):
        F = Y[col[indptr[u]:indptr[u + 1]]]
        r = val[indptr[u]:indptr[u + 1]]
        if implicit:
            A[u] = G + (F * (alpha * np.abs(r))[:, None]).T @ F
            b[u] = ((1 + alpha * np.abs(r)) * (r > 0)) @ F
        else:
            A[u] = F.T @ F
            b[u] = r @ F
        A[u] += reg * np.eye(k)
    return A, b


def solve(indptr, col, val, Y, reg, alpha, implicit):
    A, b = systems(indptr, col, val, Y, reg, alpha, implicit)
    x = np.linalg.solve(A, b[:, :, None])[:, :, 0]
    x[np.diff(indptr.cpu().numpy()) == 0] = 0
    return x


def check_half_step(x, indptr, col, val, Y, reg, alpha, implicit):
    """||A x - b||_inf <= ((3k+1) k + d + k + 2) u (||A|| ||x|| + ||b||) per
    row (Higham Thm. 10.4 plus the summation error of forming A; d is the
    degree, plus n_cols for G in implicit mode); empty rows are exactly 0."""
    A, b = systems(indptr, col, val, Y, reg, alpha, implicit)
    x = x.cpu().numpy().astype(np.float64)
    deg = np.diff(indptr.cpu().numpy())
    k = Y.shape[1]
    assert np.isfinite(x).all()
    for u in range(len(deg)):
        if deg[u] == 0:
            assert not x[u].any(), u
            continue
        d = deg[u] + (Y.shape[0] if implicit else 0)
        bound = ((3 * k + 1) * k + d + k + 2) * U32 * (
            np.abs(A[u]).sum(1).max() * np.abs(x[u]).max() + np.abs(b[u]).max())
        res = np.abs(A[u] @ x[u] - b[u]).max()
        print("row %d deg %d residual %.3e bound %.3e" % (u, deg[u], res, bound))
        assert res <= bound, (u, deg[u], res, bound)


def indexed_access_log():
    """tests/test_cyber.py's two-group log with per-tenant indices, and the
    same-group / cross-group probe frames of its separation test."""
    from mmlspark_amd.models.cyber import IdIndexer
    df = _access_log()
    for c in ("user", "res"):
        df = IdIndexer(inputCol=c, partitionKey="tenant",
                       outputCol=c + "_idx").fit(df).transform(df)
    normal = df.head(40)
    anomalous = normal.copy()
    anomalous["res_idx"] = (anomalous["res_idx"] + 10) % 20
    return df, normal, anomalous


def separates(model, normal, anomalous):
    s_norm = model.transform(normal)["anomaly_score"].to_numpy()
    s_anom = model.transform(anomalous)["anomaly_score"].to_numpy()
    return np.nanmean(s_anom) > np.nanmean(s_norm) + 0.5


def oracle_fit(n_u, n_r, u, r, y, rank, reg, iters, seed, implicit, alpha):
    """_als_csr's iteration in float64 from the same initial factors."""
    from mmlspark_amd.models.cyber import _csr
    g = torch.Generator().manual_seed(seed)
    U = (torch.randn(n_u, rank, generator=g) * 0.1).double()
    V = (torch.randn(n_r, rank, generator=g) * 0.1).double()
    if implicit:      # repeated pairs are summed, as _als_csr does
        key, inv = np.unique(np.asarray(u) * n_r + r, return_inverse=True)
        y = np.bincount(inv, weights=y)
        u, r = key // n_r, key % n_r
    u, r = torch.as_tensor(u), torch.as_tensor(r)
    y = torch.as_tensor(y, dtype=torch.float32)
    by_user, by_res = _csr(u, r, y, n_u, n_r), _csr(r, u, y, n_r, n_u)
    for _ in range(iters):
        U = torch.from_numpy(solve(*by_user, V, reg, alpha, implicit))
        V = torch.from_numpy(solve(*by_res, U, reg, alpha, implicit))
    return U.numpy(), V.numpy()
