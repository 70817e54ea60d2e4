"""Pure-torch CPU reference implementations of every device op.

These are (a) the CPU execution path for GPU-less environments and
(b) the numerics reference the HIP kernels are tested against
(tests compare HIP output to these in fp32).
"""
from __future__ import annotations

import torch


def hist_build(binned_i4: torch.Tensor, rows: torch.Tensor, grad: torch.Tensor,
               hess: torch.Tensor, n_bins: int) -> torch.Tensor:
    """Per-(feature, bin) gradient/hessian/count sums over the given rows.

    binned_i4: (ngroups, n_rows, 4) uint8 — feature-interleaved binned data,
               feature f lives at [f // 4, :, f % 4].
    rows:      (m,) int32/int64 row indices of the leaf.
    grad/hess: (n_rows,) float32.
    returns:   (ngroups*4, n_bins, 3) float32 [sum_grad, sum_hess, count].
    """
    ng = binned_i4.shape[0]
    nf = ng * 4
    r = rows.long()
    b = binned_i4[:, r, :].permute(0, 2, 1).reshape(nf, -1).long()  # (nf, m)
    g = grad[r].unsqueeze(0).expand(nf, -1)
    h = hess[r].unsqueeze(0).expand(nf, -1)
    hist = torch.zeros(nf, n_bins, 3, dtype=torch.float32, device=binned_i4.device)
    hist[:, :, 0].scatter_add_(1, b, g)
    hist[:, :, 1].scatter_add_(1, b, h)
    hist[:, :, 2].scatter_add_(1, b, torch.ones_like(g))
    return hist


def partition_rows(binned_i4: torch.Tensor, rows: torch.Tensor, feature: int,
                   threshold_bin: int):
    """Split rows into (left, right): left ⇔ bin[feature] <= threshold_bin."""
    g, j = feature // 4, feature % 4
    bins = binned_i4[g, rows.long(), j]
    mask = bins <= threshold_bin
    return rows[mask], rows[~mask]


def _go_left(xv, idx, node_threshold, cat_offset, cat_words):
    """Vectorized branch decision incl. categorical bitset nodes."""
    gl = (xv <= node_threshold[idx]) | torch.isnan(xv)
    if cat_offset is not None and cat_words is not None and cat_words.numel():
        off = cat_offset[idx].long()
        is_cat = off >= 0
        if bool(is_cat.any()):
            b = torch.nan_to_num(xv, nan=0.0).round().long().clamp(0, 255)
            widx = (off.clamp(min=0) * 8 + (b >> 5)).clamp(
                max=cat_words.numel() - 1)
            w32 = cat_words[widx].long() & 0xFFFFFFFF
            bits = (w32 >> (b & 31)) & 1
            in_range = (xv >= 0) & (xv < 256) & ~torch.isnan(xv)
            cat_left = torch.where(in_range, bits.bool(),
                                   torch.ones_like(bits, dtype=torch.bool))
            gl = torch.where(is_cat, cat_left, gl)
    return gl


def predict_forest(node_feature: torch.Tensor, node_threshold: torch.Tensor,
                   node_left: torch.Tensor, node_right: torch.Tensor,
                   node_value: torch.Tensor, tree_offsets: torch.Tensor,
                   X: torch.Tensor, n_outputs: int,
                   tree_weights: torch.Tensor = None,
                   start_tree: int = 0, num_iteration: int = -1,
                   cat_offset: torch.Tensor = None,
                   cat_words: torch.Tensor = None) -> torch.Tensor:
    """Sum of per-tree leaf values over the ensemble. Vectorized traversal.

    Flattened node arrays (concatenated trees); interior node: feature >= 0,
    go left iff X[:, feature] <= threshold or X is NaN (missing → left);
    leaf: feature == -1, value = node_value.
    Trees are laid out round-robin over outputs: tree t contributes to
    output t % n_outputs (LightGBM multiclass convention).
    returns (n, n_outputs) float32 raw scores (no base score added).
    """
    n = X.shape[0]
    n_trees = tree_offsets.numel() - 1
    end_tree = n_trees if num_iteration < 0 else min(
        n_trees, start_tree + num_iteration * n_outputs)
    T = end_tree - start_tree
    if T <= 0 or n == 0:
        return torch.zeros(n, n_outputs, dtype=torch.float32, device=X.device)
    # traverse ALL trees simultaneously: (n, T) node cursors, one vectorized
    # step per tree level instead of a python loop per tree
    bases = tree_offsets[start_tree:end_tree].long().to(X.device)  # (T,)
    idx = _traverse(node_feature, node_threshold, node_left, node_right,
                    bases, n, lambda rows, f: X[rows, f], cat_offset,
                    cat_words)
    return _sum_leaf_values(node_value[idx], tree_weights, start_tree,
                            end_tree, n_outputs)


def _traverse(node_feature, node_threshold, node_left, node_right, bases, n,
              value_of, cat_offset, cat_words) -> torch.Tensor:
    """Leaf node reached by every (row, tree): (n, T) int64 flat node ids.
    value_of(rows, f) returns the (n, T) feature values the current nodes
    test — the only place the row storage (dense / CSR) matters."""
    T = bases.numel()
    idx = bases.unsqueeze(0).expand(n, T).contiguous()
    rows = torch.arange(n, device=bases.device).unsqueeze(1).expand(n, T)
    active = node_feature[idx] >= 0
    while bool(active.any()):
        f = node_feature[idx].clamp(min=0).long()
        xv = value_of(rows, f)
        go_left = _go_left(xv, idx, node_threshold, cat_offset, cat_words)
        nxt = torch.where(go_left, node_left[idx], node_right[idx]).long()
        idx = torch.where(active, nxt + bases.unsqueeze(0), idx)
        active = node_feature[idx] >= 0
    return idx


def _sum_leaf_values(vals, tree_weights, start_tree, end_tree, n_outputs):
    n = vals.shape[0]
    if tree_weights is not None:
        vals = vals * tree_weights[start_tree:end_tree].unsqueeze(0)
    out = torch.zeros(n, n_outputs, dtype=torch.float32, device=vals.device)
    if n_outputs == 1:
        out[:, 0] = vals.sum(dim=1)
    else:
        cls = (torch.arange(start_tree, end_tree, device=vals.device)
               % n_outputs)
        out.index_add_(1, cls, vals)
    return out


def predict_leaf(node_feature, node_threshold, node_left, node_right,
                 node_leaf_index, tree_offsets, X,
                 cat_offset=None, cat_words=None) -> torch.Tensor:
    """Per-tree leaf index for each row: (n, n_trees) int32."""
    n = X.shape[0]
    n_trees = tree_offsets.numel() - 1
    if n_trees == 0 or n == 0:
        return torch.zeros(n, n_trees, dtype=torch.int32, device=X.device)
    bases = tree_offsets[:-1].long().to(X.device)
    idx = _traverse(node_feature, node_threshold, node_left, node_right,
                    bases, n, lambda rows, f: X[rows, f], cat_offset,
                    cat_words)
    return node_leaf_index[idx].to(torch.int32)


def _csr_value_of(indptr, col, val, n_cols):
    """Row accessor over CSR storage for _traverse, without densifying:
    key = row * n_cols + col is globally sorted (rows ascend, columns are
    strictly increasing within a row), so searchsorted finds the slot and an
    equality check decides the hit.  Absent entries — and split features at
    or beyond n_cols, whose key would alias the next row — read 0.0."""
    n = indptr.numel() - 1
    counts = indptr[1:] - indptr[:-1]
    erow = torch.repeat_interleave(
        torch.arange(n, device=indptr.device), counts)
    stride = max(int(n_cols), 1)
    keys = erow * stride + col.long()
    nnz = keys.numel()

    def value_of(rows, f):
        if nnz == 0:
            return torch.zeros(rows.shape, dtype=torch.float32,
                               device=val.device)
        q = (rows * stride + f).contiguous()
        slot = torch.searchsorted(keys, q).clamp(max=nnz - 1)
        hit = (keys[slot] == q) & (f < n_cols)
        return torch.where(hit, val[slot], torch.zeros((), dtype=val.dtype,
                                                       device=val.device))
    return value_of


def predict_forest_csr(node_feature, node_threshold, node_left, node_right,
                       node_value, tree_offsets, indptr, col, val, n_cols,
                       n_outputs, tree_weights=None, start_tree=0,
                       num_iteration=-1, cat_offset=None,
                       cat_words=None) -> torch.Tensor:
    """predict_forest over CSR rows (indptr int64 (n+1,), col int32 strictly
    increasing per row, val f32): an absent feature is 0.0, a stored value
    (NaN, 0.0, negative) is itself.  Same traversal and accumulation as the
    dense reference; the matrix is never densified."""
    n = indptr.numel() - 1
    n_trees = tree_offsets.numel() - 1
    end_tree = n_trees if num_iteration < 0 else min(
        n_trees, start_tree + num_iteration * n_outputs)
    if end_tree - start_tree <= 0 or n == 0:
        return torch.zeros(n, n_outputs, dtype=torch.float32,
                           device=val.device)
    bases = tree_offsets[start_tree:end_tree].long().to(val.device)
    idx = _traverse(node_feature, node_threshold, node_left, node_right,
                    bases, n, _csr_value_of(indptr, col, val, n_cols),
                    cat_offset, cat_words)
    return _sum_leaf_values(node_value[idx], tree_weights, start_tree,
                            end_tree, n_outputs)


def predict_leaf_csr(node_feature, node_threshold, node_left, node_right,
                     node_leaf_index, tree_offsets, indptr, col, val, n_cols,
                     cat_offset=None, cat_words=None) -> torch.Tensor:
    """predict_leaf over CSR rows: (n, n_trees) int32, never densified."""
    n = indptr.numel() - 1
    n_trees = tree_offsets.numel() - 1
    if n_trees == 0 or n == 0:
        return torch.zeros(n, n_trees, dtype=torch.int32, device=val.device)
    bases = tree_offsets[:-1].long().to(val.device)
    idx = _traverse(node_feature, node_threshold, node_left, node_right,
                    bases, n, _csr_value_of(indptr, col, val, n_cols),
                    cat_offset, cat_words)
    return node_leaf_index[idx].to(torch.int32)


def tree_shap_csr(node_feature, node_threshold, node_left, node_right,
                  node_value, node_count, tree_offsets, node_slot, n_slots,
                  indptr, col, val, n_cols, n_outputs, row_begin=0,
                  row_end=None, cat_offset=None, cat_words=None,
                  return_bound=False):
    """Path-dependent TreeSHAP over the CSR rows [row_begin, row_end), compact
    result: (rows, n_outputs, n_slots + 1) float64, one cell per distinct
    split feature (node_slot[node] = its index in the sorted used-feature
    list) and a last cell left 0 for the expected value.

    The float64 oracle of tree_shap_csr_k and the CPU implementation.  It
    takes the kernel's own flat float32 arrays (leaf values already folded
    with shrinkage and tree weight, float32 covers), reads row values through
    _csr_value_of, branches with _go_left (the kernels' rule) and forms each
    cover ratio as a float32 division; everything after that is float64.

    The DFS order of a tree does not depend on the row — only the
    one-fractions do — so each tree is walked once with (rows,) vectors.

    return_bound=True also returns, per output cell, N (leaf terms added
    into the cell) and S = sum |leaf value| * unwound_sum, the addends'
    magnitude without their (o - z) factor."""
    import numpy as np
    n_all = indptr.numel() - 1
    row_end = n_all if row_end is None else int(row_end)
    row_begin = int(row_begin)
    n = row_end - row_begin
    n_trees = tree_offsets.numel() - 1
    phi = np.zeros((n, n_outputs, n_slots + 1), dtype=np.float64)
    N = np.zeros(phi.shape, dtype=np.int64)
    S = np.zeros(phi.shape, dtype=np.float64)

    def result():
        out = torch.from_numpy(phi)
        if return_bound:
            return out, torch.from_numpy(N), torch.from_numpy(S)
        return out

    if n <= 0 or n_trees <= 0:
        return result()

    value_of = _csr_value_of(indptr, col, val, n_cols)
    all_rows = torch.arange(row_begin, row_end).unsqueeze(1)

    def branch_decisions(lo, hi):
        """{node: (rows,) float64 1.0 where the row goes left} for one
        tree's interior nodes, from one vectorised lookup."""
        interior = lo + torch.nonzero(node_feature[lo:hi] >= 0).view(-1)
        if not interior.numel():
            return {}
        idx = interior.unsqueeze(0).expand(n, interior.numel())
        xv = value_of(all_rows.expand(n, interior.numel()),
                      node_feature[idx].long())
        gl = _go_left(xv, idx, node_threshold, cat_offset,
                      cat_words).numpy().astype(np.float64)
        return {int(nd): gl[:, j] for j, nd in enumerate(interior.tolist())}

    feat = node_feature.numpy()
    left, right = node_left.numpy(), node_right.numpy()
    value = node_value.numpy().astype(np.float32)
    cnt = node_count.numpy().astype(np.float32)
    slot = node_slot.numpy()
    offsets = tree_offsets.numpy()
    tiny = np.float32(1e-12)

    def leaf(nd, k, path):
        # merge duplicate slots: z is a scalar, o a (rows,) 0/1 vector
        ms, mz, mo = [], [], []
        for s_, z_, o_ in path:
            if s_ in ms:
                j = ms.index(s_)
                mz[j] = mz[j] * z_
                mo[j] = mo[j] * o_
            else:
                ms.append(s_)
                mz.append(z_)
                mo.append(o_)
        m = len(ms)
        w = [np.ones(n)] + [None] * m
        for e in range(m):
            w[e + 1] = np.zeros(n)
            for i in range(e, -1, -1):
                w[i + 1] = w[i + 1] + mo[e] * w[i] * (i + 1) / (e + 2)
                w[i] = mz[e] * w[i] * (e + 1 - i) / (e + 2)
        leaf_v = float(value[nd])
        for i in range(m):
            on = mo[i] != 0.0
            safe_o = np.where(on, mo[i], 1.0)
            t_on = np.zeros(n)
            t_off = np.zeros(n)
            nrun = w[m]
            for j in range(m - 1, -1, -1):
                tmp = nrun * (m + 1) / ((j + 1) * safe_o)
                t_on = t_on + tmp
                nrun = w[j] - tmp * mz[i] * (m - j) / (m + 1)
                t_off = t_off + w[j] * (m + 1) / (mz[i] * (m - j))
            total = np.where(on, t_on, t_off)
            phi[:, k, ms[i]] += total * (mo[i] - mz[i]) * leaf_v
            N[:, k, ms[i]] += 1
            S[:, k, ms[i]] += abs(leaf_v) * np.abs(total)

    def walk(nd, base, k, path, go_left):
        if feat[nd] < 0:
            leaf(nd, k, path)
            return
        gl = go_left[nd]
        denom = np.maximum(cnt[nd], tiny)
        for child, one in ((left[nd], gl), (right[nd], 1.0 - gl)):
            c = base + int(child)
            z = float(np.float32(cnt[c]) / denom)  # the kernel's f32 ratio
            walk(c, base, k, path + [(int(slot[nd]), z, one)], go_left)

    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(n_trees):
            base, end = int(offsets[t]), int(offsets[t + 1])
            if end > base:
                walk(base, base, t % n_outputs, [],
                     branch_decisions(base, end))
    return result()


def bin_matrix(X: torch.Tensor, upper_bounds: torch.Tensor,
               n_bins: int) -> torch.Tensor:
    """Quantile-bin a dense (n, nf) matrix into the (ngroups, n, 4) i4 layout.

    upper_bounds: (nf, n_bins-1) float32 ascending per-feature boundaries
    (+inf padded). bin = searchsorted(bounds, x) so x <= bounds[b] → bin<=b.
    NaN maps to bin 0.
    """
    n, nf = X.shape
    ng = (nf + 3) // 4
    # NaN -> -inf lands in bin 0; torch.where, because nan_to_num would also
    # turn +-inf into +-FLT_MAX and move them across an infinite bound
    Xc = torch.where(torch.isnan(X), torch.full_like(X, -float("inf")), X)
    bins = torch.searchsorted(upper_bounds.contiguous(),
                              Xc.t().contiguous(), right=False)
    bins = bins.clamp(max=n_bins - 1).to(torch.uint8)  # (nf, n)
    out = torch.zeros(ng, n, 4, dtype=torch.uint8, device=X.device)
    for f in range(nf):
        out[f // 4, :, f % 4] = bins[f]
    return out


def split_scan(hists: torch.Tensor, n_bins: int, l1: float, l2: float,
               min_data: float, min_hess: float, min_gain: float,
               nf_real: int, feat_mask=None) -> torch.Tensor:
    """Best split per histogram. hists (n_hists, nf_pad, n_bins, 3) ->
    (n_hists, 6) {gain, feature, bin, GL, HL, CL}. Matches split_scan_k."""
    g = hists[..., 0]
    h = hists[..., 1]
    c = hists[..., 2]
    GL = g.cumsum(-1)
    HL = h.cumsum(-1)
    CL = c.cumsum(-1)
    G = GL[..., -1:]
    H = HL[..., -1:]
    C = CL[..., -1:]
    GR, HR, CR = G - GL, H - HL, C - CL

    def sc(Gs, Hs):
        Ga = (Gs.abs() - l1).clamp_min(0)
        return Ga * Ga / (Hs + l2 + 1e-32)

    gain = sc(GL, HL) + sc(GR, HR) - sc(G, H)
    valid = ((CL >= min_data) & (CR >= min_data)
             & (HL >= min_hess) & (HR >= min_hess))
    neg = torch.full_like(gain, float("-inf"))
    gain = torch.where(valid, gain, neg)
    gain[..., -1] = float("-inf")
    # a feature with at most one occupied bin never splits, whatever
    # min_data says (the kernel's nz_bins <= 1 shortcut; LightGBM's rule)
    degenerate = (c > 0).sum(dim=-1) <= 1
    gain = torch.where(degenerate.unsqueeze(-1), neg, gain)
    if feat_mask is not None:
        gain[:, ~feat_mask, :] = float("-inf")
    gain[:, nf_real:, :] = float("-inf")
    per_f, per_bin = gain.max(dim=-1)           # (nh, nf)
    bf = per_f.argmax(dim=-1)                   # (nh,)
    nh = hists.shape[0]
    ar = torch.arange(nh, device=hists.device)
    bb = per_bin[ar, bf]
    out = torch.stack([
        per_f[ar, bf], bf.float(), bb.float(),
        GL[ar, bf, bb], HL[ar, bf, bb], CL[ar, bf, bb]], dim=-1)
    return out


# ------------------------------------------------------------------ sparse CSR
def _expand_csr(indptr: torch.Tensor, rows: torch.Tensor):
    """(entry_indices, row_position_per_entry) for the given rows."""
    rows = rows.long()
    starts = indptr[rows]
    counts = indptr[rows + 1] - starts
    total = int(counts.sum())
    if total == 0:
        z = torch.zeros(0, dtype=torch.int64, device=indptr.device)
        return z, z
    seg = torch.repeat_interleave(starts, counts)
    off = torch.arange(total, device=indptr.device)
    bounds = torch.repeat_interleave(torch.cumsum(counts, 0) - counts, counts)
    rpos = torch.repeat_interleave(
        torch.arange(rows.numel(), device=indptr.device), counts)
    return seg + (off - bounds), rpos


def csr_hist_fixed(indptr, col, binv, gq, hq, rows, nf, n_bins):
    """Fixed-point histogram over stored CSR entries of `rows`
    (implicit zeros are corrected by the caller from exact leaf totals).
    Returns (nf, n_bins, 3) int64 — matches csr_hist_fixed_k."""
    e, rpos = _expand_csr(indptr, rows)
    hist = torch.zeros(nf * n_bins, 3, dtype=torch.int64, device=binv.device)
    if e.numel():
        r = rows.long()[rpos]
        flat = col[e].long() * n_bins + binv[e].long()
        src = torch.stack([gq[r], hq[r], torch.ones_like(gq[r])], dim=1)
        hist.index_add_(0, flat, src)
    return hist.view(nf, n_bins, 3)


def csr_gather_bins(indptr, col, binv, rows, feature: int, zero_bin: int):
    """Bin of `feature` for each row (missing → zero_bin); matches
    csr_gather_bin_k."""
    e, rpos = _expand_csr(indptr, rows)
    out = torch.full((rows.numel(),), int(zero_bin), dtype=torch.int64,
                     device=binv.device)
    if e.numel():
        m = col[e].long() == int(feature)
        out[rpos[m]] = binv[e[m]].long()
    return out


# ------------------------------------------------------------------- images
_JPEG_ZIGZAG = (
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


def _jpeg_idct_basis() -> torch.Tensor:
    """Orthonormal DCT-III basis b[x, u], computed like the host decoder."""
    import math
    b = torch.empty(8, 8, dtype=torch.float64)
    for x in range(8):
        for u in range(8):
            a = math.sqrt(1.0 / 8.0) if u == 0 else math.sqrt(2.0 / 8.0)
            b[x, u] = a * math.cos((2 * x + 1) * u * math.pi / 16.0)
    return b


def _jpeg_plane(coef, q, bw: int, bh: int, basis) -> torch.Tensor:
    """(bw*bh, 64) zigzag int16 blocks -> (bh*8, bw*8) f32 samples.  Every
    product and sum is its own rounded f64 operation, added in the host
    decoder's order (u = 0..7, then v = 0..7), so the result is the host's."""
    zz = torch.tensor(_JPEG_ZIGZAG, dtype=torch.long)
    dq = torch.zeros(coef.shape[0], 64, dtype=torch.float64)
    dq[:, zz] = coef.double() * q.double()
    dq = dq.view(-1, 8, 8)                       # [block, y, u]
    tmp = torch.zeros_like(dq)                   # [block, y, x]
    for u in range(8):
        tmp = tmp + basis[:, u].view(1, 1, 8) * dq[:, :, u].unsqueeze(2)
    px = torch.zeros_like(dq)                    # [block, y, x]
    for v in range(8):
        px = px + basis[:, v].view(1, 8, 1) * tmp[:, v, :].unsqueeze(1)
    px = (px + 128.0).float()
    return px.view(bh, bw, 8, 8).permute(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _jpeg_u8(v: torch.Tensor) -> torch.Tensor:
    return (v + 0.5).clamp(0.0, 255.0).to(torch.uint8)


def jpeg_reconstruct(coef, qt, img_desc, comp_desc, work_off, out):
    """Dequantise, IDCT, replicate chroma, convert and crop a batch of
    entropy-decoded JPEGs into `out` — matches jpeg_reconstruct_k and the
    host decoder.  Descriptor layout as in image_kernels.hip; work_off is
    the kernel's scheduling table and is not needed here."""
    basis = _jpeg_idct_basis()
    qt = qt.to(torch.int32)
    for i in range(img_desc.shape[0]):
        W, H, nc, out_off = (int(t) for t in img_desc[i])
        hmax, vmax = int(comp_desc[i, 0, 0]), int(comp_desc[i, 0, 1])
        mcux = (W + 8 * hmax - 1) // (8 * hmax)
        mcuy = (H + 8 * vmax - 1) // (8 * vmax)
        planes = []
        for c in range(nc):
            h, v, tq, off = (int(t) for t in comp_desc[i, c])
            bw, bh = mcux * h, mcuy * v
            planes.append((_jpeg_plane(coef[off:off + bw * bh], qt[i, tq],
                                       bw, bh, basis), h, v))
        if nc == 1:
            img = _jpeg_u8(planes[0][0][:H, :W])
        else:
            ys, xs = torch.arange(H), torch.arange(W)
            Y = planes[0][0][:H, :W]
            Cb, Cr = (p[(ys // (vmax // v)).unsqueeze(1),
                        (xs // (hmax // h)).unsqueeze(0)] - 128.0
                      for p, h, v in planes[1:])
            r = Y + 1.402 * Cr
            g = Y - 0.344136 * Cb - 0.714136 * Cr
            b = Y + 1.772 * Cb
            img = torch.stack([_jpeg_u8(r), _jpeg_u8(g), _jpeg_u8(b)], dim=2)
        out[out_off:out_off + img.numel()] = img.reshape(-1)
    return out


IMG_DESC_I = 24
IMG_DESC_F = 34
IMG_OP_KINDS = ("binary", "binary_inv", "trunc", "tozero", "tozero_inv",
                "normalize")


def _image_axis(dst, scale, n_in: int):
    """Taps and weights of destination indices `dst` on an axis resized
    from n_in samples with `scale` = f32(n_in) / f32(n_out): every step is
    its own rounded float32 operation, in image_preprocess_k's order."""
    import numpy as np
    half = np.float32(0.5)
    src = np.float32(scale) * (dst.astype(np.float32) + half) - half
    src = np.where(src < 0, np.float32(0), src).astype(np.float32)
    i0 = np.clip(np.floor(src).astype(np.int64), 0, n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0.astype(np.float32)
    l0 = np.float32(1.0) - l1
    return i0, i1, l0, l1


def image_preprocess(src, idesc, fdesc, work_off, out):
    """Crop / flip / bilinear resize / channel map / threshold / normalize /
    layout of a ragged image batch into `out` — numpy float32 in the order
    of the contract in docs/kernels.md, so the result has the bits
    image_preprocess_k writes.  Descriptor layout as in image_kernels.hip;
    work_off is the kernel's scheduling table and is not needed here."""
    import numpy as np
    s_all, o_all = src.numpy(), out.numpy()
    D, F = idesc.numpy(), fdesc.numpy()
    as_u8 = o_all.dtype == np.uint8
    for i in range(D.shape[0]):
        d, f = [int(t) for t in D[i]], F[i]
        src_off, Hs, Ws, Cs, py0, px0, Hc, Wc, flags = d[:9]
        qy0, qx0, Ho, Wo, Co, cmap, gmap, out_off, n_ops, kinds = d[11:21]
        img = s_all[src_off:src_off + Hs * Ws * Cs].reshape(Hs, Ws, Cs)
        ox, oy = np.arange(Wo), np.arange(Ho)
        rx = qx0 + (Wo - 1 - ox if flags & 4 else ox)
        ry = qy0 + (Ho - 1 - oy if flags & 8 else oy)

        def to_src(iy, ix):
            sy = py0 + (Hc - 1 - iy if flags & 2 else iy)
            sx = px0 + (Wc - 1 - ix if flags & 1 else ix)
            return img[sy[:, None], sx[None, :], :].astype(np.float32)

        if flags & 16:
            y0, y1, l0y, l1y = _image_axis(ry, f[0], Hc)
            x0, x1, l0x, l1x = _image_axis(rx, f[1], Wc)
            l0x, l1x = l0x[None, :, None], l1x[None, :, None]
            l0y, l1y = l0y[:, None, None], l1y[:, None, None]
            top = l0x * to_src(y0, x0) + l1x * to_src(y0, x1)
            bot = l0x * to_src(y1, x0) + l1x * to_src(y1, x1)
            s = l0y * top + l1y * bot
        else:
            s = to_src(ry, rx)
        codes = [(cmap >> (8 * k)) & 0xff for k in range(Co)]
        gray = None
        if 4 in codes:
            c0, c1, c2 = (s[:, :, (gmap >> (8 * k)) & 3] for k in range(3))
            gray = ((np.float32(0.299) * c2 + np.float32(0.587) * c1)
                    + np.float32(0.114) * c0)
        v = np.stack([gray if c >= 4 else s[:, :, c] for c in codes], axis=2)
        zero = np.float32(0)
        for j in range(n_ops):
            kind = (kinds >> (8 * j)) & 0xff
            q = f[2 + 8 * j:10 + 8 * j]
            thr, mx = q[0], q[1]
            if kind == 0:
                v = np.where(v > thr, mx, zero)
            elif kind == 1:
                v = np.where(v > thr, zero, mx)
            elif kind == 2:
                v = np.minimum(v, thr)
            elif kind == 3:
                v = np.where(v > thr, v, zero)
            elif kind == 4:
                v = np.where(v > thr, zero, v)
            elif kind == 5:
                v = (v / np.float32(255.0) - q[None, None, :Co]) \
                    / q[None, None, 4:4 + Co]
            v = v.astype(np.float32, copy=False)
        if as_u8:
            v = np.clip(v, 0, 255).astype(np.uint8)
        if flags & 32:
            v = v.transpose(2, 0, 1)
        o_all[out_off:out_off + Ho * Wo * Co] = v.reshape(-1)
    return out


# ------------------------------------------------------------------ ranking
def group_rank(score: torch.Tensor, offsets: torch.Tensor, gid: torch.Tensor,
               label: torch.Tensor, gain: torch.Tensor,
               disc_tbl: torch.Tensor):
    """Stable descending rank of every document inside its query group, and
    the per-document records lambdarank_grad reads — matches group_rank_k.

    rank[i] counts the documents j of i's group with
    s_j > s_i or (s_j == s_i and j < i), so it equals the inverse of
    np.argsort(-s, kind="stable") per group and lies in [0, m) for any
    scores.  Generic in dtype: the records take score's dtype.
    returns (rank (n,) int32, records (n, 4) [s, label, gain, disc_tbl[rank]]).
    """
    n = score.numel()
    dt = score.dtype
    rank = torch.zeros(n, dtype=torch.int64)
    offs = offsets.tolist()
    for b, e in zip(offs[:-1], offs[1:]):
        if e - b <= 1:
            continue
        s = score[b:e]
        idx = torch.arange(e - b)
        ahead = (s.unsqueeze(0) > s.unsqueeze(1)) | (
            (s.unsqueeze(0) == s.unsqueeze(1))
            & (idx.unsqueeze(0) < idx.unsqueeze(1)))
        rank[b:e] = ahead.sum(dim=1)
    rec = torch.stack([score, label.to(dt), gain.to(dt),
                       disc_tbl.to(dt)[rank]], dim=1)
    return rank.to(torch.int32), rec


def lambdarank_grad(records: torch.Tensor, offsets: torch.Tensor,
                    gid: torch.Tensor, inv_idcg: torch.Tensor, sigma: float):
    """Lambdarank gradient and hessian per document — matches
    lambdarank_grad_k, in the dtype of `records` (float32 is the kernel's
    reference, float64 an evaluation of the same formulas).

    Over every j of i's group with label_i != label_j, hi being the one with
    the larger label and x = sigma * (s_hi - s_lo):
      e = exp(-|x|), q = 1 / (1 + e), rho = q if x < 0 else e * q
      delta = |gain_i - gain_j| * |disc_i - disc_j| * inv_idcg[group]
      g_i -= sigma * rho * delta if i is hi else += ;
      h_i += sigma^2 * (e * q * q) * delta
    Groups of size 0 or 1 and documents without such a partner get exactly 0.
    """
    n = records.shape[0]
    g = torch.zeros(n, dtype=records.dtype)
    h = torch.zeros(n, dtype=records.dtype)
    inv = inv_idcg.to(records.dtype)
    offs = offsets.tolist()
    for k, (b, e) in enumerate(zip(offs[:-1], offs[1:])):
        if e - b <= 1:
            continue
        s, y, gn, d = records[b:e].unbind(dim=1)
        differ = y.unsqueeze(1) != y.unsqueeze(0)
        i_hi = y.unsqueeze(1) > y.unsqueeze(0)
        ds = s.unsqueeze(1) - s.unsqueeze(0)
        x = sigma * torch.where(i_hi, ds, -ds)
        ex = torch.exp(-x.abs())
        q = 1.0 / (1.0 + ex)
        eq = ex * q
        rho = torch.where(x < 0, q, eq)
        delta = ((gn.unsqueeze(1) - gn.unsqueeze(0)).abs()
                 * (d.unsqueeze(1) - d.unsqueeze(0)).abs() * inv[k])
        t = sigma * rho * delta
        zero = torch.zeros_like(t)
        g[b:e] = torch.where(differ, torch.where(i_hi, -t, t), zero).sum(dim=1)
        h[b:e] = torch.where(differ, (sigma * sigma) * (eq * q) * delta,
                             zero).sum(dim=1)
    return g, h


# ------------------------------------------------------- nearest neighbours
def _knn_allowed(label_ids, allow_bits, lo, hi):
    """(hi - lo, n) bool: bit label_ids[j] of query i's bitset, the words
    read as unsigned."""
    lid = label_ids.long()
    words = allow_bits[lo:hi].long()[:, lid >> 5] & 0xFFFFFFFF
    return ((words >> (lid & 31).unsqueeze(0)) & 1).bool()


def _knn_select(d2, k):
    """First k of every row under (d2 ascending, index ascending); slots
    whose distance is +inf become (+inf, -1)."""
    srt, order = torch.sort(d2, dim=1, stable=True)
    srt, order = srt[:, :k], order[:, :k]
    pad = k - srt.shape[1]
    if pad > 0:
        srt = torch.nn.functional.pad(srt, (0, pad), value=float("inf"))
        order = torch.nn.functional.pad(order, (0, pad), value=-1)
    order = torch.where(torch.isinf(srt) & (srt > 0),
                        torch.full_like(order, -1), order)
    return srt, order.to(torch.int32)


def _knn_run(Q, X, k, label_ids, allow_bits, dist_fn, dtype, row_cost):
    n_q = Q.shape[0]
    out_d = torch.full((n_q, k), float("inf"), dtype=dtype)
    out_i = torch.full((n_q, k), -1, dtype=torch.int32)
    if X.shape[0] == 0:
        return out_d, out_i
    step = max(1, (1 << 24) // max(1, row_cost))
    for lo in range(0, n_q, step):
        hi = min(n_q, lo + step)
        d2 = dist_fn(Q[lo:hi])
        if label_ids is not None:
            d2 = torch.where(_knn_allowed(label_ids, allow_bits, lo, hi), d2,
                             torch.full_like(d2, float("inf")))
        out_d[lo:hi], out_i[lo:hi] = _knn_select(d2, k)
    return out_d, out_i


def knn_topk(Q, X, xsq, k, label_ids=None, allow_bits=None, splits=0):
    """The k nearest index rows of every query under the total order
    (d2 ascending, index ascending) — the contract of knn_partial_topk_k +
    knn_merge_k, in float32 with torch's GEMM: d2 = (xsq - 2 q.x) + ||q||^2,
    unclamped.  A point whose label bit is not set in the query's bitset
    (allow_bits (n_q, W) int32, read as unsigned) is left out; a query with
    fewer than k allowed points gets (+inf, -1) in the remaining slots.
    `splits` only shapes the device launch.  Returns (d2 (n_q, k) float32,
    idx (n_q, k) int32)."""
    def dist(q):
        return (xsq.unsqueeze(0) - 2.0 * (q @ X.t())) \
            + (q * q).sum(1, keepdim=True)
    return _knn_run(Q, X, k, label_ids, allow_bits, dist, torch.float32,
                    X.shape[0])


def knn_topk_f64(Q, X, k, label_ids=None, allow_bits=None):
    """knn_topk's answer from float64 distances sum((q - x)^2): the exact
    order on integer data.  Returns (D (n_q, k) float64, idx int32)."""
    Xd = X.double()

    def dist(q):
        diff = q.double().unsqueeze(1) - Xd.unsqueeze(0)
        return (diff * diff).sum(2)
    return _knn_run(Q, Xd, k, label_ids, allow_bits, dist, torch.float64,
                    X.shape[0] * X.shape[1])


# ------------------------------------------------------------ recommendation
# Sparse SAR in torch ops on whatever device the CSR arrays live on: the
# contract of ops/hip/sar_kernels.hip (int64 indptr, int32 columns strictly
# increasing per row, float32 values).
def _csr_rows(indptr):
    """Row index of every stored entry."""
    n = indptr.numel() - 1
    return torch.repeat_interleave(
        torch.arange(n, device=indptr.device), indptr[1:] - indptr[:-1])


def _expand_segments(starts, lengths):
    """For segments (starts[s], lengths[s]): the owner s of every element and
    its absolute position, segments in order."""
    dev = starts.device
    owner = torch.repeat_interleave(
        torch.arange(lengths.numel(), device=dev), lengths)
    first = torch.cumsum(lengths, 0) - lengths
    pos = starts[owner] + (torch.arange(owner.numel(), device=dev)
                           - first[owner])
    return owner, pos


def sar_cooccurrence(b_indptr, b_col, bt_indptr, bt_col, threshold, sim,
                     tile=0):
    """S = similarity(Bt.B) as CSR.  c_ij = users holding both items,
    occ_i = c_ii; an entry is kept iff c_ij >= threshold (>= 1), diagonal
    included.  sim 0: (float)c; 1 (jaccard): (float)c / (float)(occ_i + occ_j
    - c); 2 (lift): (float)c / ((float)occ_i * (float)occ_j).  The pairs of
    a chunk of users are enumerated and counted with torch.unique, so memory
    follows sum(deg^2) of a chunk, never items^2.  `tile` only shapes the
    device launch.  Returns (indptr int64, col int32, val float32)."""
    dev = b_col.device
    n_users, n_items = b_indptr.numel() - 1, bt_indptr.numel() - 1
    deg = b_indptr[1:] - b_indptr[:-1]
    occ = bt_indptr[1:] - bt_indptr[:-1]
    csum = torch.cumsum(deg * deg, 0)
    keys, cnts = [], []
    lo = 0
    while lo < n_users:
        base = int(csum[lo - 1]) if lo else 0
        hi = int(torch.searchsorted(csum, torch.tensor(base + (1 << 24),
                                                       device=dev),
                                    right=True))
        hi = min(n_users, max(hi, lo + 1))
        e = torch.arange(int(b_indptr[lo]), int(b_indptr[hi]), device=dev)
        user = lo + _csr_rows(b_indptr[lo:hi + 1] - b_indptr[lo])
        owner, pos = _expand_segments(b_indptr[user], deg[user])
        key = b_col[e[owner]].long() * n_items + b_col[pos].long()
        uk, c = torch.unique(key, return_counts=True)
        keys.append(uk)
        cnts.append(c)
        lo = hi
    if keys:
        uk, inv = torch.unique(torch.cat(keys), return_inverse=True)
        c = torch.zeros(uk.numel(), dtype=torch.int64, device=dev)
        c.index_add_(0, inv, torch.cat(cnts))
    else:
        uk = torch.zeros(0, dtype=torch.int64, device=dev)
        c = uk
    keep = c >= max(int(threshold), 1)
    uk, c = uk[keep], c[keep]
    i, j = uk // max(n_items, 1), uk % max(n_items, 1)
    val = c.float()
    if sim == 1:
        val = val / (occ[i] + occ[j] - c).float()
    elif sim == 2:
        val = val / (occ[i].float() * occ[j].float())
    indptr = torch.zeros(n_items + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(i, minlength=n_items), 0)
    return indptr, j.to(torch.int32), val


def sar_recommend(a_indptr, a_col, a_val, s_indptr, s_col, s_val, users, k,
                  remove_seen=True, tile=0):
    """Top-k items of every requested user (all when `users` is None) under
    the total order (score descending, item ascending).  score(u, j) = sum
    over u's stored entries i of a_ui * s_ij, float32; with remove_seen the
    items whose affinity is > 0 are no candidates, every other item is, zero
    scores included.  Users are scored in chunks densified by index_add_
    (its order of addition is torch's, not the kernel's ascending-i fmaf
    chain).  Returns (items (n, k) int32, scores (n, k) float32) with
    (-1, -inf) in unused slots."""
    dev = a_col.device
    n_users, n_items = a_indptr.numel() - 1, s_indptr.numel() - 1
    rows = (torch.arange(n_users, device=dev) if users is None
            else users.long())
    n = rows.numel()
    out_i = torch.full((n, k), -1, dtype=torch.int32, device=dev)
    out_s = torch.full((n, k), float("-inf"), dtype=torch.float32, device=dev)
    if n == 0 or n_items == 0:
        return out_i, out_s
    s_len = s_indptr[1:] - s_indptr[:-1]
    kk = min(k, n_items)
    step = max(1, (1 << 24) // n_items)
    for lo in range(0, n, step):
        r = rows[lo:lo + step]
        m = r.numel()
        own, e = _expand_segments(a_indptr[r], a_indptr[r + 1] - a_indptr[r])
        it, av = a_col[e].long(), a_val[e]
        own2, q = _expand_segments(s_indptr[it], s_len[it])
        sc = torch.zeros(m * n_items, dtype=torch.float32, device=dev)
        sc.index_add_(0, own[own2] * n_items + s_col[q].long(),
                      av[own2] * s_val[q])
        if remove_seen:
            seen = av > 0
            sc[own[seen] * n_items + it[seen]] = float("-inf")
        srt, order = torch.sort(sc.view(m, n_items), dim=1, descending=True,
                                stable=True)
        srt, order = srt[:, :kk], order[:, :kk]
        gone = torch.isinf(srt) & (srt < 0)
        out_s[lo:lo + m, :kk] = srt
        out_i[lo:lo + m, :kk] = torch.where(
            gone, torch.full_like(order, -1), order).to(torch.int32)
    return out_i, out_s


def sar_score_pairs(a_indptr, a_col, a_val, s_indptr, s_col, s_val, users,
                    items):
    """score(u, i) of sar_recommend for every (users[p], items[p]); a pair
    with an id out of range scores 0.  float32 (n,)."""
    dev = a_col.device
    n_users, n_items = a_indptr.numel() - 1, s_indptr.numel() - 1
    out = torch.zeros(users.numel(), dtype=torch.float32, device=dev)
    u, i = users.long(), items.long()
    idx = torch.nonzero((u >= 0) & (u < n_users) & (i >= 0) & (i < n_items)
                        ).flatten()
    if idx.numel() == 0 or s_col.numel() == 0:
        return out
    skey = _csr_rows(s_indptr) * n_items + s_col.long()
    step = 1 << 20
    for lo in range(0, idx.numel(), step):
        sel = idx[lo:lo + step]
        uu, ii = u[sel], i[sel]
        own, e = _expand_segments(a_indptr[uu], a_indptr[uu + 1] - a_indptr[uu])
        want = ii[own] * n_items + a_col[e].long()
        pos = torch.searchsorted(skey, want).clamp_(max=skey.numel() - 1)
        hit = skey[pos] == want
        part = torch.zeros(sel.numel(), dtype=torch.float32, device=dev)
        part.index_add_(0, own[hit], a_val[e][hit] * s_val[pos[hit]])
        out[sel] = part
    return out
