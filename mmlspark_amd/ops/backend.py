"""Device-op dispatch: HIP/CDNA4 extension on GPU tensors, torch reference on CPU.

The HIP extension is built IN-TREE (mmlspark_amd/ops/_hip_ops*.so) by
``python setup.py build_ext --inplace`` / ``__graft_entry__.build()`` so the
.so travels to the GPU box with the repo snapshot.  On a CUDA/ROCm tensor the
extension is REQUIRED — a missing .so raises instead of silently falling back
to eager torch (the round-end check records which native libraries the GPU
processes actually loaded).
"""
from __future__ import annotations

import torch

from . import cpu_ref

_EXT = None
_EXT_ERR: str = ""


def _load_ext():
    global _EXT, _EXT_ERR
    if _EXT is not None:
        return _EXT
    try:
        from . import _hip_ops  # built in-tree
        _EXT = _hip_ops
    except ImportError as e:
        _EXT_ERR = str(e)
        _EXT = False
    return _EXT


def hip_available() -> bool:
    return bool(_load_ext()) and torch.cuda.is_available()


def _require_ext():
    ext = _load_ext()
    if not ext:
        raise RuntimeError(
            "mmlspark_amd HIP extension is required for GPU tensors but is not "
            "built (import error: %s). Run `python setup.py build_ext --inplace` "
            "(PYTORCH_ROCM_ARCH=gfx950)." % _EXT_ERR)
    return ext


# --------------------------------------------------------------------------- GBDT
def hist_build(binned_i4, rows, grad, hess, n_bins):
    if binned_i4.is_cuda:
        return _require_ext().hist_build(binned_i4, rows, grad, hess, n_bins)
    return cpu_ref.hist_build(binned_i4, rows, grad, hess, n_bins)


def hist_build_fixed_pair(binned_pair, rows, grad, hess, n_bins, tail_bytes,
                          scale_g, scale_h):
    """Fixed-point histogram over PAIRED planes ((npairs, n) int64: two
    uchar4 feature groups per element — one cacheline per gathered row).
    tail_bytes = valid feature-bytes in the last pair (zero-pad skipped).
    GPU-only (the pairing exists only on the device path)."""
    return _require_ext().hist_build_fixed_pair(binned_pair, rows, grad,
                                                hess, n_bins, tail_bytes,
                                                scale_g, scale_h)


def hist_build_fixed(binned_i4, rows, grad, hess, n_bins, scale_g, scale_h):
    """Fixed-point int64 histogram (GPU; 9x faster integer LDS atomics).
    Returns (nf_pad, n_bins, 3) int64: [g*scale_g, h*scale_h, count]."""
    if binned_i4.is_cuda:
        return _require_ext().hist_build_fixed(binned_i4, rows, grad, hess,
                                               n_bins, scale_g, scale_h)
    h = cpu_ref.hist_build(binned_i4, rows, grad, hess, n_bins)
    scale = torch.tensor([scale_g, scale_h, 1.0])
    return (h.double() * scale).round().long()


def partition_rows(binned_i4, rows, feature, threshold_bin, known_left=-1):
    if binned_i4.is_cuda:
        # ordered 3-kernel partition; ONE device→host sync, or zero when the
        # caller already knows the left count (single-rank training)
        return _require_ext().partition_rows(binned_i4, rows.contiguous(),
                                             feature, threshold_bin,
                                             known_left)
    return cpu_ref.partition_rows(binned_i4, rows, feature, threshold_bin)


def predict_forest(node_feature, node_threshold, node_left, node_right,
                   node_value, tree_offsets, X, n_outputs,
                   tree_weights=None, start_tree=0, num_iteration=-1,
                   cat_offset=None, cat_words=None):
    if X.is_cuda:
        n_trees = tree_offsets.numel() - 1
        end_tree = n_trees if num_iteration < 0 else min(
            n_trees, start_tree + num_iteration * n_outputs)
        if tree_weights is None:
            tree_weights = torch.ones(n_trees, dtype=torch.float32, device=X.device)
        return _require_ext().predict_forest(
            node_feature, node_threshold, node_left, node_right, node_value,
            tree_offsets, tree_weights, X, n_outputs, start_tree, end_tree,
            cat_offset, cat_words)
    return cpu_ref.predict_forest(node_feature, node_threshold, node_left,
                                  node_right, node_value, tree_offsets, X,
                                  n_outputs, tree_weights, start_tree,
                                  num_iteration, cat_offset, cat_words)


def predict_leaf(node_feature, node_threshold, node_left, node_right,
                 node_leaf_index, tree_offsets, X,
                 cat_offset=None, cat_words=None):
    if X.is_cuda:
        return _require_ext().predict_leaf(
            node_feature, node_threshold, node_left, node_right,
            node_leaf_index, tree_offsets, X, cat_offset, cat_words)
    return cpu_ref.predict_leaf(node_feature, node_threshold, node_left,
                                node_right, node_leaf_index, tree_offsets, X,
                                cat_offset, cat_words)


def split_scan(hists, n_bins, l1, l2, min_data, min_hess, min_gain, nf_real,
               feat_mask=None):
    if hists.is_cuda:
        return _require_ext().split_scan(hists.contiguous(), n_bins, l1, l2,
                                         min_data, min_hess, min_gain,
                                         nf_real, feat_mask)
    return cpu_ref.split_scan(hists, n_bins, l1, l2, min_data, min_hess,
                              min_gain, nf_real, feat_mask)


def sibling_scan(parent, small, small_is_left, n_bins, l1, l2, min_data,
                 min_hess, nf_real, feat_mask=None, scale_g=1.0, scale_h=1.0):
    """The native grower's split scan (sibling_scan_k) on fixed-point int64
    histograms (nf_pad, n_bins, 3) = [g*scale_g, h*scale_h, count].  With
    `parent`, the other child's histogram big = parent - small is formed
    and scanned in the same launch: returns (records (2, nf_pad, 6), big),
    record row 0 the left child's and row 1 the right child's.  Without it
    `small` is scanned alone: (records (1, nf_pad, 6), None).  A record is
    one feature's {gain, feature, bin, GL, HL, CL}; the arg-max over
    features (lowest feature on ties) is the caller's.  GPU-only."""
    if not small.is_cuda:
        raise RuntimeError("sibling_scan runs on the GPU only")
    _require_ext()
    from . import _hip_grower
    return _hip_grower.sibling_scan(parent, small, bool(small_is_left),
                                    int(n_bins), l1, l2, min_data, min_hess,
                                    int(nf_real), feat_mask, scale_g, scale_h)


def bin_matrix(X, upper_bounds, n_bins):
    if X.is_cuda:
        return _require_ext().bin_matrix(X, upper_bounds, n_bins)
    return cpu_ref.bin_matrix(X, upper_bounds, n_bins)


# --------------------------------------------------------------------------- VW
def vw_sgd_minibatch(indices, values, offsets, labels, weights_tbl, adaptive_tbl,
                     lr, l2, power_t, loss: str, ex_weight=None,
                     normalize_tbl=None, invariant=False):
    if weights_tbl.is_cuda:
        return _require_ext().vw_sgd_minibatch(
            indices, values, offsets, labels, weights_tbl, adaptive_tbl,
            lr, l2, power_t, {"squared": 0, "logistic": 1, "hinge": 2}[loss],
            ex_weight, normalize_tbl, invariant)
    from ..models.vw import sgd_ref
    return sgd_ref.vw_sgd_minibatch(indices, values, offsets, labels,
                                    weights_tbl, adaptive_tbl, lr, l2,
                                    power_t, loss, ex_weight, normalize_tbl,
                                    invariant)


def vw_predict(indices, values, offsets, weights_tbl):
    if weights_tbl.is_cuda:
        return _require_ext().vw_predict(indices, values, offsets, weights_tbl)
    from ..models.vw import sgd_ref
    return sgd_ref.vw_predict(indices, values, offsets, weights_tbl)


# --------------------------------------------------------------- sparse CSR
def csr_hist_fixed(indptr, col, binv, gq, hq, rows, nf, n_bins):
    """Fixed-point histogram over STORED entries of `rows` from a binned CSR
    shard; (nf, n_bins, 3) int64.  Implicit-zero correction is the caller's
    (exact integer subtraction from leaf totals)."""
    if binv.is_cuda:
        return _require_ext().csr_hist_fixed(indptr, col, binv, gq, hq,
                                             rows.contiguous(), nf, n_bins)
    return cpu_ref.csr_hist_fixed(indptr, col, binv, gq, hq, rows, nf, n_bins)


def csr_gather_bins(indptr, col, binv, rows, feature, zero_bin):
    """Per-row bin of `feature` (missing → zero_bin) from a binned CSR shard."""
    if binv.is_cuda:
        return _require_ext().csr_gather_bins(indptr, col, binv,
                                              rows.contiguous(), feature,
                                              zero_bin).long()
    return cpu_ref.csr_gather_bins(indptr, col, binv, rows, feature, zero_bin)


def csr_hist_fixed_tot(indptr, col, binv, gq, hq, rows, nf, n_bins):
    """Histogram over stored entries PLUS exact integer leaf totals
    (sum gq, sum hq, count) in one launch — (hist, tot).  GPU: the
    wave-cooperative v2 kernel; CPU: reference + torch sums."""
    if binv.is_cuda:
        return _require_ext().csr_hist_fixed_tot(indptr, col, binv, gq, hq,
                                                 rows.contiguous(), nf,
                                                 n_bins)
    h = cpu_ref.csr_hist_fixed(indptr, col, binv, gq, hq, rows, nf, n_bins)
    r = rows.long()
    tot = torch.stack([gq[r].sum(), hq[r].sum(),
                       torch.tensor(int(rows.numel()), dtype=torch.int64)])
    return h, tot


def csr_partition_rows(indptr, col, binv, rows, feature, zero_bin,
                       threshold_bin, known_left=-1):
    """Stable ordered partition of a CSR shard's row list by one feature's
    bin (missing → zero_bin): fused predicate + 3-kernel partition on GPU,
    gather + boolean masks on CPU."""
    if binv.is_cuda:
        return _require_ext().csr_partition_rows(
            indptr, col, binv, rows.contiguous(), feature, zero_bin,
            threshold_bin, known_left)
    bins = cpu_ref.csr_gather_bins(indptr, col, binv, rows, feature, zero_bin)
    mask = bins <= threshold_bin
    return rows[mask], rows[~mask]


def predict_forest_csr(node_feature, node_threshold, node_left, node_right,
                       node_value, tree_offsets, indptr, col, val, n_cols,
                       n_outputs, tree_weights=None, start_tree=0,
                       num_iteration=-1, cat_offset=None, cat_words=None):
    """predict_forest over float CSR rows (col strictly increasing per row;
    absent feature = 0.0) — the matrix is never densified.  n_cols is the
    matrix width; a split feature at or beyond it is simply absent."""
    if val.is_cuda:
        n_trees = tree_offsets.numel() - 1
        end_tree = n_trees if num_iteration < 0 else min(
            n_trees, start_tree + num_iteration * n_outputs)
        if tree_weights is None:
            tree_weights = torch.ones(n_trees, dtype=torch.float32,
                                      device=val.device)
        return _require_ext().predict_forest_csr(
            node_feature, node_threshold, node_left, node_right, node_value,
            tree_offsets, tree_weights, indptr, col, val, n_outputs,
            start_tree, end_tree, cat_offset, cat_words)
    return cpu_ref.predict_forest_csr(
        node_feature, node_threshold, node_left, node_right, node_value,
        tree_offsets, indptr, col, val, n_cols, n_outputs, tree_weights,
        start_tree, num_iteration, cat_offset, cat_words)


def predict_leaf_csr(node_feature, node_threshold, node_left, node_right,
                     node_leaf_index, tree_offsets, indptr, col, val, n_cols,
                     cat_offset=None, cat_words=None):
    if val.is_cuda:
        return _require_ext().predict_leaf_csr(
            node_feature, node_threshold, node_left, node_right,
            node_leaf_index, tree_offsets, indptr, col, val, cat_offset,
            cat_words)
    return cpu_ref.predict_leaf_csr(
        node_feature, node_threshold, node_left, node_right, node_leaf_index,
        tree_offsets, indptr, col, val, n_cols, cat_offset, cat_words)


def tree_shap_csr(node_feature, node_threshold, node_left, node_right,
                  node_value, node_count, tree_offsets, node_slot, n_slots,
                  indptr, col, val, n_cols, n_outputs, max_depth,
                  row_begin=0, row_end=None, max_blocks=0, cat_offset=None,
                  cat_words=None):
    """TreeSHAP over the CSR rows [row_begin, row_end) — compact float32
    (rows, n_outputs, n_slots + 1): one cell per distinct split feature
    (node_slot maps an interior node to it), the last cell left 0 for the
    expected value.  node_value holds the leaf values already folded with
    the tree weights, node_count the float32 covers.  max_depth (< 32)
    picks the kernel's depth template; max_blocks > 0 overrides its grid
    policy."""
    if row_end is None:
        row_end = indptr.numel() - 1
    if val.is_cuda:
        return _require_ext().tree_shap_csr(
            node_feature, node_threshold, node_left, node_right, node_value,
            node_count, tree_offsets, node_slot, n_slots, indptr, col, val,
            n_outputs, max_depth, row_begin, row_end, max_blocks, cat_offset,
            cat_words)
    return cpu_ref.tree_shap_csr(
        node_feature, node_threshold, node_left, node_right, node_value,
        node_count, tree_offsets, node_slot, n_slots, indptr, col, val,
        n_cols, n_outputs, row_begin, row_end, cat_offset,
        cat_words).to(torch.float32)


# ------------------------------------------------------------------ ranking
def group_rank(score, offsets, gid, label, gain, disc_tbl):
    """Stable descending rank of each document inside its query group
    ((n,) int32, equal to the inverse of np.argsort(-s, kind="stable") per
    group) and the (n, 4) records [s, label, gain, disc_tbl[rank]] that
    lambdarank_grad reads.  offsets (G+1) int64, gid (n) int32; the group
    table is validated where it is built (models/gbdt/ranking.py)."""
    if score.is_cuda:
        return _require_ext().group_rank(score, offsets, gid, label, gain,
                                         disc_tbl)
    return cpu_ref.group_rank(score, offsets, gid, label, gain, disc_tbl)


def lambdarank_grad(records, offsets, gid, inv_idcg, sigma):
    """Lambdarank (g, h) per document from group_rank's records, every query
    group in one launch; inv_idcg (G) is the reciprocal ideal DCG per group.
    Unclamped and unweighted: the objective does both afterwards."""
    if records.is_cuda:
        return _require_ext().lambdarank_grad(records, offsets, gid, inv_idcg,
                                              float(sigma))
    return cpu_ref.lambdarank_grad(records, offsets, gid, inv_idcg,
                                   float(sigma))


# ------------------------------------------------------- nearest neighbours
KNN_MAX_K = 64        # knn_partial_topk_k keeps k <= 64 pairs per query in LDS
KNN_MAX_SPLITS = 64   # knn_merge_k holds splits * k pairs in LDS


def check_knn_inputs(Q, X, xsq, k, label_ids, allow_bits, splits):
    """Everything the knn kernels index with, checked in O(inputs); raises
    ValueError and nothing is launched."""
    def bad(msg):
        raise ValueError("knn_topk: " + msg)

    for name, t in (("Q", Q), ("X", X), ("xsq", xsq)):
        if t.dtype != torch.float32:
            bad(name + " must be float32")
        if not t.is_contiguous():
            bad(name + " must be contiguous")
        if t.device != X.device:
            bad(name + " must live where X lives")
    if Q.dim() != 2 or X.dim() != 2 or X.shape[1] < 1 \
            or Q.shape[1] != X.shape[1]:
        bad("Q (n_q, d) and X (n, d) must agree on d >= 1")
    n_q, n = Q.shape[0], X.shape[0]
    if n >= (1 << 31):
        bad("n_index must be below 2^31")
    if xsq.dim() != 1 or xsq.shape[0] != n:
        bad("xsq must hold one squared norm per index row")
    if not 1 <= int(k) <= KNN_MAX_K:
        bad("k must be in [1, %d]" % KNN_MAX_K)
    if not 0 <= int(splits) <= KNN_MAX_SPLITS:
        bad("splits must be in [0, %d] (0 = automatic)" % KNN_MAX_SPLITS)
    if (label_ids is None) != (allow_bits is None):
        bad("label_ids and allow_bits must be given together")
    if label_ids is None:
        return
    for name, t in (("label_ids", label_ids), ("allow_bits", allow_bits)):
        if t.dtype != torch.int32:
            bad(name + " must be int32")
        if not t.is_contiguous():
            bad(name + " must be contiguous")
        if t.device != X.device:
            bad(name + " must live where X lives")
    if label_ids.dim() != 1 or label_ids.shape[0] != n:
        bad("label_ids must hold one label id per index row")
    if allow_bits.dim() != 2 or allow_bits.shape[0] != n_q \
            or allow_bits.shape[1] < 1:
        bad("allow_bits must be (n_q, W) with W >= 1")
    if n and (int(label_ids.min()) < 0
              or int(label_ids.max()) >= 32 * allow_bits.shape[1]):
        bad("label_ids must lie in [0, 32 * W)")


def knn_topk(Q, X, xsq, k, label_ids=None, allow_bits=None, splits=0):
    """Exact k nearest index rows of every query, 1 <= k <= KNN_MAX_K, under
    the total order (squared distance ascending, index ascending).

    Q (n_q, d), X (n, d), xsq (n) = row sums of X*X, all float32.  With
    label_ids (n) int32 and allow_bits (n_q, W) int32, point j is a candidate
    for query i only if bit label_ids[j] of row i is set (word label >> 5,
    bit label & 31, words read as unsigned).  splits > 0 fixes how many
    pieces the index is cut into on the device; the result does not depend
    on it.  Returns (d2 (n_q, k) float32 = ||q||^2 - 2 q.x + ||x||^2,
    unclamped, idx (n_q, k) int32); a query with fewer than k candidates has
    (+inf, -1) in its last slots."""
    check_knn_inputs(Q, X, xsq, k, label_ids, allow_bits, splits)
    if X.is_cuda:
        return _require_ext().knn_topk(Q, X, xsq, int(k), label_ids,
                                       allow_bits, int(splits))
    return cpu_ref.knn_topk(Q, X, xsq, int(k), label_ids, allow_bits,
                            int(splits))


# ------------------------------------------------------------ recommendation
SAR_MAX_K = 128        # sar_recommend_topk_k keeps 2k (score, item) pairs in LDS
SAR_MAX_TILE = 16384   # LDS cells of one item tile
SAR_SIMILARITY = {"cooccurrence": 0, "jaccard": 1, "lift": 2}


def check_sar_csr(name, indptr, col, val, n_cols, structure=True):
    """A CSR matrix as the sar kernels read it: int64 indptr (rows + 1),
    int32 col, float32 val (None for a pattern), all contiguous and on one
    device.  With `structure` also everything the kernels index with, in
    O(nnz) on the device: indptr from 0 to nnz without decreasing, columns
    inside [0, n_cols) and strictly increasing inside a row, values finite.
    Raises ValueError; nothing is launched."""
    def bad(msg):
        raise ValueError("sar: %s %s" % (name, msg))

    tensors = [("indptr", indptr, torch.int64), ("col", col, torch.int32)]
    if val is not None:
        tensors.append(("val", val, torch.float32))
    for what, t, dt in tensors:
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            bad("%s must be a %s tensor" % (what, str(dt).split(".")[-1]))
        if t.dim() != 1 or not t.is_contiguous():
            bad(what + " must be 1-D and contiguous")
        if t.device != indptr.device:
            bad(what + " must live where indptr lives")
    if indptr.numel() < 1:
        bad("indptr must hold rows + 1 entries")
    if indptr.numel() - 1 >= (1 << 31) or int(n_cols) >= (1 << 31):
        bad("must have fewer than 2^31 rows and columns")
    if val is not None and val.numel() != col.numel():
        bad("val must hold one value per column index")
    if not structure:
        return
    nnz = col.numel()
    if int(indptr[0]) != 0 or int(indptr[-1]) != nnz:
        bad("indptr must start at 0 and end at nnz")
    if indptr.numel() > 1 and bool((indptr[1:] < indptr[:-1]).any()):
        bad("indptr must not decrease")
    if nnz:
        if int(col.min()) < 0 or int(col.max()) >= int(n_cols):
            bad("columns must lie in [0, %d)" % int(n_cols))
        rising = col[1:] > col[:-1]
        starts = indptr[1:-1]
        starts = starts[(starts > 0) & (starts < nnz)]
        rising[starts - 1] = True
        if not bool(rising.all()):
            bad("columns must be strictly increasing inside a row")
        if val is not None and not bool(torch.isfinite(val).all()):
            bad("values must be finite")


def _check_sar_tile(tile):
    if int(tile) != tile or tile < 0 or tile % 64 or tile > SAR_MAX_TILE:
        raise ValueError("sar: tile must be 0 (automatic) or a multiple of 64 "
                         "up to %d" % SAR_MAX_TILE)
    return int(tile)


def _sar_fused(t) -> bool:
    """GPU tensors go to sar_kernels.hip unless MMLSPARK_AMD_SAR_FUSED=0."""
    import os
    return t.is_cuda and os.environ.get("MMLSPARK_AMD_SAR_FUSED", "1") != "0"


def sar_cooccurrence(b_indptr, b_col, bt_indptr, bt_col, threshold,
                     similarity, tile=0, check=True):
    """Item-item similarity of a binarised user-item CSR pattern B (users x
    items) and its transpose Bt, as CSR (indptr int64, col int32 ascending,
    val float32), symmetric, diagonal included.  c_ij = users holding both
    items, occ_i = c_ii; an entry is kept iff c_ij >= max(threshold, 1).
    similarity: "cooccurrence" (float)c, "jaccard" (float)c / (float)(occ_i +
    occ_j - c), "lift" (float)c / ((float)occ_i * (float)occ_j), IEEE float32.
    `tile` (a multiple of 64, 0 = automatic) is the item-tile width of the
    device kernels; the result does not depend on it.  check=False skips the
    O(nnz) structure check for patterns already checked."""
    if similarity not in SAR_SIMILARITY:
        raise ValueError("sar: similarity must be one of %s"
                         % sorted(SAR_SIMILARITY))
    tile = _check_sar_tile(tile)
    n_users, n_items = b_indptr.numel() - 1, bt_indptr.numel() - 1
    check_sar_csr("B", b_indptr, b_col, None, n_items, check)
    check_sar_csr("Bt", bt_indptr, bt_col, None, n_users, check)
    if bt_col.device != b_col.device or bt_col.numel() != b_col.numel():
        raise ValueError("sar: B and Bt must hold the same entries on one "
                         "device")
    thr = min(max(int(threshold), 1), (1 << 31) - 1)
    sim = SAR_SIMILARITY[similarity]
    if _sar_fused(b_col):
        return _require_ext().sar_cooccurrence(b_indptr, b_col, bt_indptr,
                                               bt_col, thr, sim, tile)
    return cpu_ref.sar_cooccurrence(b_indptr, b_col, bt_indptr, bt_col, thr,
                                    sim, tile)


def _check_sar_model(a_indptr, a_col, a_val, s_indptr, s_col, s_val, check):
    n_items = s_indptr.numel() - 1
    check_sar_csr("affinity", a_indptr, a_col, a_val, n_items, check)
    check_sar_csr("similarity", s_indptr, s_col, s_val, n_items, check)
    if s_col.device != a_col.device:
        raise ValueError("sar: affinity and similarity must share a device")


def _check_sar_ids(name, t, like):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise ValueError("sar: %s must be an int32 tensor" % name)
    if t.dim() != 1 or not t.is_contiguous():
        raise ValueError("sar: %s must be 1-D and contiguous" % name)
    if t.device != like.device:
        raise ValueError("sar: %s must live where the model lives" % name)


def sar_recommend(a_indptr, a_col, a_val, s_indptr, s_col, s_val, users, k,
                  remove_seen=True, tile=0, check=True):
    """The k best items of every user in `users` ((n,) int32, repeats allowed;
    None = every user) from CSR affinity (users x items) and similarity (items
    x items): score(u, j) = sum_i a_ui * s_ij, ordered by (score descending,
    item ascending).  Every item is a candidate, zero scores included, except,
    with remove_seen, those whose affinity is > 0.  On the device a score is
    the fmaf chain over the user's entries in ascending i from 0.0f, whatever
    `tile` is.  k above SAR_MAX_K, CPU tensors and MMLSPARK_AMD_SAR_FUSED=0
    take cpu_ref.sar_recommend.  Returns (items (n, k) int32, scores (n, k)
    float32), (-1, -inf) in unused slots."""
    if int(k) != k or k < 1:
        raise ValueError("sar: k must be an integer >= 1")
    tile = _check_sar_tile(tile)
    _check_sar_model(a_indptr, a_col, a_val, s_indptr, s_col, s_val, check)
    if users is not None:
        _check_sar_ids("users", users, a_col)
        n_users = a_indptr.numel() - 1
        if users.numel() and (int(users.min()) < 0
                              or int(users.max()) >= n_users):
            raise ValueError("sar: users must lie in [0, %d)" % n_users)
    if _sar_fused(a_col) and k <= SAR_MAX_K:
        return _require_ext().sar_recommend(a_indptr, a_col, a_val, s_indptr,
                                            s_col, s_val, users, int(k),
                                            bool(remove_seen), tile)
    return cpu_ref.sar_recommend(a_indptr, a_col, a_val, s_indptr, s_col,
                                 s_val, users, int(k), bool(remove_seen), tile)


def sar_score_pairs(a_indptr, a_col, a_val, s_indptr, s_col, s_val, users,
                    items, check=True):
    """score(users[p], items[p]) as sar_recommend defines it, float32 (n,);
    on the device bit-equal to the score sar_recommend reports for that pair.
    A pair with an id outside the model scores 0."""
    _check_sar_model(a_indptr, a_col, a_val, s_indptr, s_col, s_val, check)
    _check_sar_ids("users", users, a_col)
    _check_sar_ids("items", items, a_col)
    if users.numel() != items.numel():
        raise ValueError("sar: users and items must pair up")
    if _sar_fused(a_col):
        return _require_ext().sar_score_pairs(a_indptr, a_col, a_val,
                                              s_indptr, s_col, s_val, users,
                                              items)
    return cpu_ref.sar_score_pairs(a_indptr, a_col, a_val, s_indptr, s_col,
                                   s_val, users, items)


# ------------------------------------------------------------------- images
JPEG_MAX_PIXELS = 1 << 26


def jpeg_work_items(W, H, hmax, vmax):
    """Work items (workgroups) jpeg_reconstruct_k spends on one image: a run
    of G = max(1, 4 // (hmax*vmax)) MCUs each.  Works on ints and arrays."""
    mcux = (W + 8 * hmax - 1) // (8 * hmax)
    mcuy = (H + 8 * vmax - 1) // (8 * vmax)
    G = 4 // (hmax * vmax)
    G = G + (G < 1)
    return ((mcux + G - 1) // G) * mcuy


def check_jpeg_descriptors(n_blocks, qt, img_desc, comp_desc, work_off,
                           out_bytes):
    """Validate a batch's descriptors against the buffer sizes — everything
    jpeg_reconstruct_k indexes with.  O(N) on CPU tensors; raises ValueError
    and nothing is launched.  Runs before the GPU launch and before the CPU
    reference alike."""
    import numpy as np

    def bad(msg):
        raise ValueError("jpeg_reconstruct: " + msg)

    for name, t in (("img_desc", img_desc), ("comp_desc", comp_desc),
                    ("work_off", work_off)):
        if t.is_cuda or t.dtype != torch.int64:
            bad(name + " must be a CPU int64 tensor")
    n = img_desc.shape[0] if img_desc.dim() == 2 else -1
    if (n < 0 or tuple(img_desc.shape) != (n, 4)
            or tuple(comp_desc.shape) != (n, 3, 4)
            or tuple(work_off.shape) != (n + 1,)
            or tuple(qt.shape) != (n, 4, 64)):
        bad("descriptor shapes do not agree on the batch size")
    if n == 0:
        return
    d = img_desc.numpy()
    cd = comp_desc.numpy()
    wo = work_off.numpy()
    W, H, nc, out_off = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    if ((W < 1) | (H < 1) | (W > 65535) | (H > 65535)).any() \
            or (W * H > JPEG_MAX_PIXELS).any():
        bad("image size out of range")
    if (~np.isin(nc, (1, 3))).any():
        bad("component count must be 1 or 3")
    hmax, vmax = cd[:, 0, 0], cd[:, 0, 1]
    if ((hmax < 1) | (hmax > 4) | (vmax < 1) | (vmax > 4)).any():
        bad("sampling factor out of range")
    mcux = (W + 8 * hmax - 1) // (8 * hmax)
    mcuy = (H + 8 * vmax - 1) // (8 * vmax)
    for c in range(3):
        used = nc > c
        h, v, tq, off = (np.where(used, cd[:, c, k], (1, 1, 0, 0)[k])
                         for k in range(4))
        if ((h < 1) | (h > 4) | (v < 1) | (v > 4)).any():
            bad("sampling factor out of range")
        if ((hmax % h != 0) | (vmax % v != 0)).any():
            bad("sampling factor does not divide component 0's")
        if ((tq < 0) | (tq > 3)).any():
            bad("quantisation table id above 3")
        if ((off < 0) | (off + mcux * h * mcuy * v > n_blocks))[used].any():
            bad("component blocks run past the coefficient buffer")
    if ((out_off < 0) | (out_off + H * W * nc > out_bytes)).any():
        bad("image pixels run past the output buffer")
    items = jpeg_work_items(W, H, hmax, vmax)
    if wo[0] != 0 or (np.diff(wo) != items).any():
        bad("work_off is not the prefix sum of the per-image work items")
    if wo[-1] >= (1 << 31):
        bad("batch too large for one launch")


def jpeg_reconstruct(coef, qt, img_desc, comp_desc, work_off, out):
    """Reconstruct a batch of entropy-decoded JPEGs into the uint8 buffer
    `out` (dequant, IDCT, chroma replication, YCbCr->RGB, crop) in one
    launch.  coef (blocks, 64) int16 and qt (N, 4, 64) uint16 live where
    `out` lives; the three descriptor tensors (layout in image_kernels.hip)
    are CPU int64: they are checked against the buffer sizes here, then
    copied to the device.  Pin them to make that copy asynchronous."""
    if coef.dim() != 2 or coef.shape[1] != 64 or coef.dtype != torch.int16 \
            or qt.dtype != torch.uint16 or out.dtype != torch.uint8 \
            or out.dim() != 1:
        raise ValueError("jpeg_reconstruct: coef must be (blocks, 64) int16, "
                         "qt uint16 and out a flat uint8 buffer")
    if coef.device != out.device or qt.device != out.device:
        raise ValueError("jpeg_reconstruct: coef, qt and out must share a "
                         "device")
    check_jpeg_descriptors(coef.shape[0], qt, img_desc, comp_desc, work_off,
                           out.numel())
    if out.is_cuda:
        ext = _require_ext()
        dev = out.device
        ext.jpeg_reconstruct(
            coef.contiguous(), qt.contiguous(),
            img_desc.to(dev, non_blocking=True),
            comp_desc.to(dev, non_blocking=True),
            work_off.to(dev, non_blocking=True), int(work_off[-1]), out)
        return out
    return cpu_ref.jpeg_reconstruct(coef, qt, img_desc, comp_desc, work_off,
                                    out)


IMG_TILE_W, IMG_TILE_H = 64, 8          # image_preprocess_k's output tile
IMG_DESC_I, IMG_DESC_F = cpu_ref.IMG_DESC_I, cpu_ref.IMG_DESC_F
IMG_MAX_DIM = 32768


def image_work_items(Ho, Wo):
    """Work items (workgroups) image_preprocess_k spends on one Ho x Wo
    output: tiles of 64 x 8 pixels.  Works on ints and arrays."""
    return (((Wo + IMG_TILE_W - 1) // IMG_TILE_W)
            * ((Ho + IMG_TILE_H - 1) // IMG_TILE_H))


def check_image_descriptors(src, idesc, fdesc, work_off, out):
    """Validate a batch's plan against the buffers — everything
    image_preprocess_k indexes with (descriptor layout in
    image_kernels.hip).  O(N) on CPU tensors; raises ValueError and nothing
    is launched.  Runs before the GPU launch and before the CPU reference
    alike."""
    import numpy as np

    def bad(msg):
        raise ValueError("image_preprocess: " + msg)

    for name, t in (("src", src), ("out", out)):
        if t.dtype not in (torch.uint8, torch.float32) or t.dim() != 1 \
                or not t.is_contiguous():
            bad(name + " must be a flat contiguous uint8 or float32 buffer")
    if src.device != out.device:
        bad("src and out must share a device")
    for name, t, dt in (("idesc", idesc, torch.int64),
                        ("fdesc", fdesc, torch.float32),
                        ("work_off", work_off, torch.int64)):
        if t.is_cuda or t.dtype != dt or not t.is_contiguous():
            bad(name + " must be a contiguous CPU %s tensor"
                % str(dt).replace("torch.", ""))
    n = idesc.shape[0] if idesc.dim() == 2 else -1
    if (n < 0 or tuple(idesc.shape) != (n, IMG_DESC_I)
            or tuple(fdesc.shape) != (n, IMG_DESC_F)
            or tuple(work_off.shape) != (n + 1,)):
        bad("descriptor shapes do not agree on the batch size")
    if n == 0:
        return
    d, f, wo = idesc.numpy(), fdesc.numpy(), work_off.numpy()
    (src_off, Hs, Ws, Cs, py0, px0, Hc, Wc, flags, Hr, Wr, qy0, qx0, Ho, Wo,
     Co, cmap, gmap, out_off, n_ops, kinds) = (d[:, k] for k in range(21))
    dims = np.stack([Hs, Ws, Hc, Wc, Hr, Wr, Ho, Wo])
    if ((dims < 1) | (dims > IMG_MAX_DIM)).any():
        bad("image dimension outside 1..%d" % IMG_MAX_DIM)
    if ((Cs < 1) | (Cs > 4) | (Co < 1) | (Co > 4)).any():
        bad("channel count outside 1..4")
    if ((flags < 0) | (flags > 63)).any() or (d[:, 21:] != 0).any():
        bad("unknown flag bits")
    if ((src_off < 0) | (src_off + Hs * Ws * Cs > src.numel())).any():
        bad("source image runs past the source buffer")
    if ((py0 < 0) | (px0 < 0) | (py0 + Hc > Hs) | (px0 + Wc > Ws)).any():
        bad("pre-window outside its source image")
    rs = (flags & 16) != 0
    if ((~rs) & ((Hr != Hc) | (Wr != Wc))).any():
        bad("copy path needs the resized size to equal the pre-window's")
    sy = Hc.astype(np.float32) / Hr.astype(np.float32)
    sx = Wc.astype(np.float32) / Wr.astype(np.float32)
    if (rs & ((f[:, 0] != sy) | (f[:, 1] != sx))).any():
        bad("scale is not float32(n_in) / float32(n_out)")
    if ((qy0 < 0) | (qx0 < 0) | (qy0 + Ho > Hr) | (qx0 + Wo > Wr)).any():
        bad("post-window outside the resized image")
    uses_gray = np.zeros(n, bool)
    for k in range(4):
        code = (cmap >> (8 * k)) & 0xff
        used = Co > k
        uses_gray |= used & (code == 4)
        if (used & (code != 4) & (code >= Cs)).any() \
                or (~used & (code != 0)).any():
            bad("channel map names a channel the source does not have")
    if ((cmap < 0) | (cmap >= 1 << 32) | (gmap < 0) | (gmap >= 1 << 24)).any():
        bad("channel map names a channel the source does not have")
    for k in range(3):
        if (uses_gray & (((gmap >> (8 * k)) & 0xff) >= Cs)).any():
            bad("channel map names a channel the source does not have")
    if ((n_ops < 0) | (n_ops > 4) | (kinds < 0) | (kinds >= 1 << 32)).any():
        bad("bad pointwise op table")
    for j in range(4):
        kind = (kinds >> (8 * j)) & 0xff
        if ((n_ops > j) & (kind > 5)).any() or ((n_ops <= j) & (kind != 0)).any():
            bad("bad pointwise op table")
    size = Ho * Wo * Co
    if ((out_off < 0) | (out_off + size > out.numel())).any():
        bad("output image runs past the output buffer")
    if ((out_off * out.element_size()) % 4 != 0).any():
        bad("output image does not start on a dword")
    order = np.argsort(out_off, kind="stable")
    if (out_off[order][1:] < (out_off + size)[order][:-1]).any():
        bad("output images overlap")
    if wo[0] != 0 or (np.diff(wo) != image_work_items(Ho, Wo)).any():
        bad("work_off is not the prefix sum of the per-image work items")
    if wo[-1] >= (1 << 31):
        bad("batch too large for one launch")


def image_preprocess(src, idesc, fdesc, work_off, out):
    """Run a compiled image plan (models/images.py::compile_image_plan) over
    the flat source buffer `src` into the flat buffer `out`, one launch for
    the whole batch.  src / out are uint8 or float32 and share a device; the
    descriptor tensors are CPU tensors: they are checked against the buffers
    here, then copied to the device.  Pin them to make that copy
    asynchronous."""
    check_image_descriptors(src, idesc, fdesc, work_off, out)
    if out.is_cuda:
        ext = _require_ext()
        dev = out.device
        ext.image_preprocess(
            src, idesc.to(dev, non_blocking=True),
            fdesc.to(dev, non_blocking=True),
            work_off.to(dev, non_blocking=True), int(work_off[-1]), out)
        return out
    return cpu_ref.image_preprocess(src, idesc, fdesc, work_off, out)
