"""Sparse CSR GBDT on MI355X: kernel numerics vs CPU reference + the
high-dimensional training run that is out of reach for the dense path."""
import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs ROCm GPU")


def _dense_of(rows, nf):
    X = np.zeros((len(rows), nf), dtype=np.float32)
    for i, v in enumerate(rows):
        X[i, v.indices] = v.values
    return X


def _rand_csr(gen, n, nf, nnz_per_row):
    counts = torch.randint(0, nnz_per_row * 2, (n,), generator=gen)
    indptr = torch.zeros(n + 1, dtype=torch.int64)
    indptr[1:] = counts.cumsum(0)
    nnz = int(indptr[-1])
    col = torch.empty(nnz, dtype=torch.int32)
    for i in range(n):  # sorted unique columns per row
        c = int(counts[i])
        if c:
            col[indptr[i]:indptr[i + 1]] = torch.randperm(
                nf, generator=gen)[:c].sort().values.to(torch.int32)
    binv = torch.randint(0, 31, (nnz,), generator=gen, dtype=torch.uint8)
    return indptr, col, binv


@requires_gpu
def test_csr_hist_kernel_matches_cpu():
    from mmlspark_amd.ops import backend, cpu_ref
    gen = torch.Generator().manual_seed(0)
    n, nf, nb = 50_000, 300, 31
    indptr, col, binv = _rand_csr(gen, n, nf, 12)
    gq = torch.randint(-2**40, 2**40, (n,), generator=gen, dtype=torch.int64)
    hq = torch.randint(0, 2**24, (n,), generator=gen, dtype=torch.int64)
    rows = torch.randperm(n, generator=gen)[: n // 3].to(
        torch.int32).sort().values
    ref = cpu_ref.csr_hist_fixed(indptr, col, binv, gq, hq, rows, nf, nb)
    out, _ = backend.csr_hist_fixed_tot(indptr.cuda(), col.cuda(),
                                        binv.cuda(), gq.cuda(), hq.cuda(),
                                        rows.cuda(), nf, nb)
    assert torch.equal(out.cpu(), ref)  # integer atomics: exact


@requires_gpu
def test_sparse_gpu_training_matches_cpu():
    """End-to-end sparse training GPU vs CPU: identical int64 histograms on
    both sides ⇒ identical tree STRUCTURE; leaf values differ only in final
    ulps (the GPU split scan is a Hillis-Steele parallel float reduction,
    the CPU reference a sequential cumsum)."""
    from mmlspark_amd.core.schema import SparseVector
    from mmlspark_amd.models.gbdt.estimators import LightGBMClassifier
    rng = np.random.default_rng(4)
    n, nf = 6000, 60
    rows, y = [], np.zeros(n, dtype=np.float32)
    w = rng.normal(size=nf)
    for i in range(n):
        idx = np.sort(rng.choice(nf, size=10, replace=False)).astype(np.int32)
        val = rng.normal(size=10).astype(np.float32)
        y[i] = 1.0 if (w[idx] * val).sum() > 0 else 0.0
        rows.append(SparseVector(nf, idx, val))
    df = pd.DataFrame({"features": rows, "label": y})
    from sklearn.metrics import roc_auc_score
    m_cpu = LightGBMClassifier(numIterations=10, numLeaves=15,
                               device="cpu").fit(df)
    m_gpu = LightGBMClassifier(numIterations=10, numLeaves=15,
                               device="cuda").fit(df)
    X = torch.from_numpy(_dense_of(rows, nf))
    p_cpu = m_cpu.booster.predict_raw(X).squeeze(-1).numpy()
    p_gpu = m_gpu.booster.predict_raw(X).squeeze(-1).numpy()
    # same algorithm, same binning; the GPU split scan is a parallel float
    # reduction so an exact-tie argmax can flip — match the dense parity
    # test's quality-based comparison (test_gpu_cpu_training_parity)
    a_cpu = roc_auc_score(y, p_cpu)
    a_gpu = roc_auc_score(y, p_gpu)
    assert abs(a_cpu - a_gpu) < 0.01, (a_cpu, a_gpu)
    assert np.corrcoef(p_cpu, p_gpu)[0, 1] > 0.99


@requires_gpu
@pytest.mark.timeout(600)
def test_sparse_high_dim_1m_x_100k():
    """1M×100k sparse trains within memory budget.
    Dense binned storage would need 100 GB+ of uint8 alone; CSR is ~1 GB."""
    from mmlspark_amd.models.gbdt.objectives import make_objective
    from mmlspark_amd.models.gbdt.sparse import CsrMatrix
    from mmlspark_amd.models.gbdt.trainer import TrainConfig, train_booster
    from mmlspark_amd.parallel.comm import Comm

    gen = torch.Generator().manual_seed(9)
    n, nf, nnz = 1_000_000, 100_000, 20
    # synthetic CSR straight on device: random sorted columns per row
    col = torch.randint(0, nf, (n * nnz,), generator=gen,
                        dtype=torch.int32).view(n, nnz).sort(dim=1).values
    val = torch.randn(n * nnz, generator=gen)
    indptr = torch.arange(0, (n + 1) * nnz, nnz, dtype=torch.int64)
    w = torch.randn(nf, generator=gen)
    contrib = w[col.view(-1).long()].view(n, nnz) * val.view(n, nnz)
    y = (contrib.sum(dim=1) > 0).float()
    csr = CsrMatrix(indptr.cuda(), col.view(-1).cuda(), val.cuda(), (n, nf))
    yt = y.cuda()
    free0, total = torch.cuda.mem_get_info()
    cfg = TrainConfig(num_iterations=3, num_leaves=15, max_bin=15,
                      min_data_in_leaf=50, bin_sample_count=50_000)
    booster, stats = train_booster(csr, yt, cfg, make_objective("binary"),
                                   Comm())
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"[sparse 1Mx100k] peak alloc {peak/2**30:.2f} GiB, "
          f"hist {stats.hist_s:.2f}s total {stats.total_s:.2f}s")
    assert booster.num_trees == 3
    assert peak < 40 * 2**30  # far under the 100 GB+ a dense path would need


@requires_gpu
def test_csr_hist_v2_fused_totals_matches_cpu():
    """Wave-cooperative kernels (LDS row staging + in-kernel totals) must
    be integer-exact vs the reference, including ragged tails.  nf <= 2048
    runs csr_hist_fixed_lds_k, wider nf runs csr_hist_fixed_v2_k; a third of
    the n rows are selected, so n = 900 gives 300: one full 256-row block
    and a second whose waves hold 44, 0, 0 and 0 rows."""
    from mmlspark_amd.ops import backend, cpu_ref
    gen = torch.Generator().manual_seed(7)
    for n, nf, nb, nnz in ((50_000, 300, 31, 12), (4097, 64, 255, 3),
                           (63, 10, 15, 5), (300, 2048, 15, 5),
                           (300, 2049, 15, 5), (63, 4096, 15, 5),
                           (900, 2049, 15, 5)):
        indptr, col, binv = _rand_csr(gen, n, nf, nnz)
        binv = (binv % nb).contiguous()  # bins must lie in [0, nb)
        gq = torch.randint(-2**40, 2**40, (n,), generator=gen,
                           dtype=torch.int64)
        hq = torch.randint(0, 2**24, (n,), generator=gen, dtype=torch.int64)
        rows = torch.randperm(n, generator=gen)[: max(1, n // 3)].to(
            torch.int32).sort().values
        ref = cpu_ref.csr_hist_fixed(indptr, col, binv, gq, hq, rows, nf, nb)
        r = rows.long()
        ref_tot = torch.stack([gq[r].sum(), hq[r].sum(),
                               torch.tensor(int(rows.numel()),
                                            dtype=torch.int64)])
        out, tot = backend.csr_hist_fixed_tot(
            indptr.cuda(), col.cuda(), binv.cuda(), gq.cuda(), hq.cuda(),
            rows.cuda(), nf, nb)
        assert torch.equal(out.cpu(), ref), (n, nf)
        assert torch.equal(tot.cpu(), ref_tot), (n, tot.cpu(), ref_tot)


@requires_gpu
def test_csr_partition_rows_kernel_matches_cpu():
    """Fused CSR partition (predicate + stable ordered split) == the CPU
    gather+mask reference, including the known-left no-sync path."""
    from mmlspark_amd.ops import backend
    gen = torch.Generator().manual_seed(21)
    n, nf, nb = 70_000, 150, 63
    indptr, col, binv = _rand_csr(gen, n, nf, 9)
    binv = (binv % nb).contiguous()
    rows = torch.randperm(n, generator=gen)[: n // 2].to(
        torch.int32).sort().values
    for f, zb, thr in ((3, 5, 20), (149, 0, 0), (80, 31, 62)):
        ref_l, ref_r = backend.csr_partition_rows(
            indptr, col, binv, rows, f, zb, thr)
        got_l, got_r = backend.csr_partition_rows(
            indptr.cuda(), col.cuda(), binv.cuda(), rows.cuda(), f, zb, thr)
        assert torch.equal(got_l.cpu(), ref_l), (f, thr)
        assert torch.equal(got_r.cpu(), ref_r), (f, thr)
        gl2, gr2 = backend.csr_partition_rows(
            indptr.cuda(), col.cuda(), binv.cuda(), rows.cuda(), f, zb, thr,
            known_left=ref_l.numel())
        assert torch.equal(gl2.cpu(), ref_l)
        assert torch.equal(gr2.cpu(), ref_r)
