// Python bindings for the MI355X HIP kernels (pure-ROCm torch extension —
// no hipify, no CUDA shims: this file uses torch's native c10::hip API and
// links the hipcc-compiled kernel objects).
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#define CHECK_DEV(x) TORCH_CHECK(x.is_cuda(), #x " must be on the GPU")
#define CHECK_CONTIG(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

extern "C" {
void launch_hist_build(const void*, long, const int*, long, const float*,
                       const float*, float*, int, int, hipStream_t);
void launch_predict_forest(const int*, const float*, const int*, const int*,
                           const float*, const long*, const float*,
                           const float*, long, int, float*, int, int, int,
                           const int*, const unsigned*, hipStream_t);
void launch_predict_leaf(const int*, const float*, const int*, const int*,
                         const int*, const long*, const float*, long, int,
                         int*, int, const int*, const unsigned*, hipStream_t);
void launch_predict_forest_csr(const int*, const float*, const int*,
                               const int*, const float*, const long*,
                               const float*, const long*, const int*,
                               const float*, long, float*, int, int, int,
                               const int*, const unsigned*, hipStream_t);
void launch_predict_leaf_csr(const int*, const float*, const int*, const int*,
                             const int*, const long*, const long*, const int*,
                             const float*, long, int*, int, const int*,
                             const unsigned*, hipStream_t);
void launch_bin_matrix(const float*, const float*, long, int, int, int, void*,
                       hipStream_t);
void launch_hist_build_fixed(const void*, long, const int*, long, const float*,
                             const float*, long long*, int, int, double,
                             double, hipStream_t);
void launch_hist_build_fixed_pair(const void*, long, const int*, long,
                                  const float*, const float*, const void*,
                                  long long*, int, int, int, double, double,
                                  const int*, int, hipStream_t);
void launch_partition(const void*, long, const int*, long, int, int, int*,
                      int*, int*, hipStream_t);
void launch_split_scan(const float*, int, long, int, float, float, float,
                       float, long, const bool*, float*, float*, hipStream_t);
void launch_vw_sgd(const int*, const float*, const long*, const float*,
                   const float*, float*, float*, float*, float, float, float,
                   int, int, long, float*, hipStream_t);
void launch_vw_predict(const int*, const float*, const long*, const float*,
                       long, float*, hipStream_t);
void launch_tree_shap(const int*, const float*, const int*, const int*,
                      const float*, const float*, const long*, const int*,
                      const unsigned*, const float*, long, int, int, int, int,
                      float*, hipStream_t);
void launch_tree_shap_csr(const int*, const float*, const int*, const int*,
                          const float*, const float*, const long*, const int*,
                          const int*, const unsigned*, const long*, const int*,
                          const float*, long, long, int, int, int, int, float*,
                          long, hipStream_t);
void launch_csr_hist_fixed(const long*, const int*,
                           const unsigned char*, const long long*,
                           const long long*, const int*, long, long long*,
                           int, hipStream_t);
void launch_csr_gather_bin(const long*, const int*, const unsigned char*,
                           const int*, long, int, int, int*, hipStream_t);
void launch_csr_hist_fixed_v2(const long*, const int*, const unsigned char*,
                              const long long*, const long long*, const int*,
                              long, long long*, int, long long*, hipStream_t);
void launch_csr_hist_fixed_lds(const long*, const int*, const unsigned char*,
                               const long long*, const long long*,
                               const int*, long, long long*, int, int,
                               long long*, hipStream_t);
void launch_csr_partition(const long*, const int*, const unsigned char*,
                          const int*, long, int, int, int, const unsigned*,
                          unsigned char*, int*, int*, int*, hipStream_t);
void launch_jpeg_reconstruct(const short*, const unsigned short*, const long*,
                             const long*, const long*, int, long,
                             unsigned char*, hipStream_t);
long image_work_items(long, long);
void launch_image_preprocess(const void*, long, int, const long*, const float*,
                             const long*, int, long, void*, long, int,
                             hipStream_t);
void launch_group_rank(const float*, const long*, const int*, const float*,
                       const float*, const float*, long, int, long, int*,
                       void*, hipStream_t);
void launch_lambdarank_grad(const void*, const long*, const int*,
                            const float*, float, long, int, float*, float*,
                            hipStream_t);
int knn_choose_splits(long, long, int, int);
int launch_knn_topk(const float*, const float*, const float*, const float*,
                    const int*, const unsigned*, long, long, int, int, int,
                    int, float*, int*, float*, int*, hipStream_t);
int sar_default_tile(long, int);
int launch_sar_cooc_count(const long*, const int*, const long*, const int*,
                          int, int, int, unsigned, int*, hipStream_t);
int launch_sar_cooc_fill(const long*, const int*, const long*, const int*, int,
                         int, int, unsigned, int, const long*, long, int*,
                         float*, hipStream_t);
int launch_sar_recommend(const long*, const int*, const float*, const long*,
                         const int*, const float*, const int*, long, int, int,
                         int, int, int, float*, int*, hipStream_t);
int launch_sar_score_pairs(const long*, const int*, const float*, const long*,
                           const int*, const float*, const int*, const int*,
                           long, int, int, float*, hipStream_t);
}

static hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

torch::Tensor hist_build(torch::Tensor binned_i4, torch::Tensor rows,
                         torch::Tensor grad, torch::Tensor hess, long n_bins) {
  CHECK_DEV(binned_i4); CHECK_CONTIG(binned_i4);
  CHECK_DEV(rows); CHECK_CONTIG(rows);
  CHECK_DEV(grad); CHECK_CONTIG(grad);
  CHECK_DEV(hess); CHECK_CONTIG(hess);
  TORCH_CHECK(binned_i4.dtype() == torch::kUInt8, "binned must be uint8");
  TORCH_CHECK(rows.dtype() == torch::kInt32, "rows must be int32");
  const long ngroups = binned_i4.size(0);
  const long n_rows = binned_i4.size(1);
  auto hist = torch::zeros({ngroups * 4, n_bins, 3},
                           grad.options().dtype(torch::kFloat32));
  launch_hist_build(binned_i4.data_ptr(), n_rows, rows.data_ptr<int>(),
                    rows.numel(), grad.data_ptr<float>(),
                    hess.data_ptr<float>(), hist.data_ptr<float>(),
                    (int)n_bins, (int)ngroups, cur_stream());
  return hist;
}

torch::Tensor hist_build_fixed_pair(torch::Tensor binned_pair,
                                    torch::Tensor rows, torch::Tensor grad,
                                    torch::Tensor hess, long n_bins,
                                    long tail_bytes,
                                    double scale_g, double scale_h) {
  CHECK_DEV(binned_pair); CHECK_CONTIG(binned_pair);
  CHECK_DEV(rows); CHECK_CONTIG(rows);
  TORCH_CHECK(rows.dtype() == torch::kInt32, "rows must be int32");
  TORCH_CHECK(binned_pair.dtype() == torch::kInt64, "paired binned is int64");
  const long npairs = binned_pair.size(0);
  const long n_rows = binned_pair.size(1);
  auto hist = torch::zeros({npairs * 8, n_bins, 3},
                           grad.options().dtype(torch::kInt64));
  launch_hist_build_fixed_pair(binned_pair.data_ptr(), n_rows,
                               rows.data_ptr<int>(), rows.numel(),
                               grad.data_ptr<float>(), hess.data_ptr<float>(),
                               nullptr,
                               (long long*)hist.data_ptr<int64_t>(),
                               (int)n_bins, (int)npairs, (int)tail_bytes,
                               scale_g, scale_h, nullptr, -1, cur_stream());
  return hist;
}

torch::Tensor hist_build_fixed(torch::Tensor binned_i4, torch::Tensor rows,
                               torch::Tensor grad, torch::Tensor hess,
                               long n_bins, double scale_g, double scale_h) {
  CHECK_DEV(binned_i4); CHECK_CONTIG(binned_i4);
  CHECK_DEV(rows); CHECK_CONTIG(rows);
  TORCH_CHECK(rows.dtype() == torch::kInt32, "rows must be int32");
  const long ngroups = binned_i4.size(0);
  const long n_rows = binned_i4.size(1);
  auto hist = torch::zeros({ngroups * 4, n_bins, 3},
                           grad.options().dtype(torch::kInt64));
  launch_hist_build_fixed(binned_i4.data_ptr(), n_rows, rows.data_ptr<int>(),
                          rows.numel(), grad.data_ptr<float>(),
                          hess.data_ptr<float>(),
                          (long long*)hist.data_ptr<int64_t>(), (int)n_bins,
                          (int)ngroups, scale_g, scale_h, cur_stream());
  return hist;
}

static std::pair<const int*, const unsigned*> cat_ptrs(
    const c10::optional<torch::Tensor>& cat_offset,
    const c10::optional<torch::Tensor>& cat_words) {
  const int* co = nullptr;
  const unsigned* cw = nullptr;
  if (cat_offset.has_value() && cat_words.has_value()
      && cat_words->numel() > 0) {
    co = cat_offset->data_ptr<int>();
    cw = (const unsigned*)cat_words->data_ptr<int>();
  }
  return {co, cw};
}

torch::Tensor predict_forest(torch::Tensor feat, torch::Tensor thr,
                             torch::Tensor left, torch::Tensor right,
                             torch::Tensor val, torch::Tensor offsets,
                             torch::Tensor tw, torch::Tensor X,
                             long n_outputs, long t0, long t1,
                             c10::optional<torch::Tensor> cat_offset,
                             c10::optional<torch::Tensor> cat_words) {
  CHECK_DEV(X); CHECK_CONTIG(X);
  const long n = X.size(0);
  const long nf = X.size(1);
  auto out = torch::zeros({n, n_outputs}, X.options().dtype(torch::kFloat32));
  TORCH_CHECK(offsets.dtype() == torch::kInt64, "offsets must be int64");
  auto [co, cw] = cat_ptrs(cat_offset, cat_words);
  launch_predict_forest(feat.data_ptr<int>(), thr.data_ptr<float>(),
                        left.data_ptr<int>(), right.data_ptr<int>(),
                        val.data_ptr<float>(), offsets.data_ptr<long>(),
                        tw.data_ptr<float>(), X.data_ptr<float>(), n, (int)nf,
                        out.data_ptr<float>(), (int)n_outputs, (int)t0,
                        (int)t1, co, cw, cur_stream());
  return out;
}

torch::Tensor predict_leaf(torch::Tensor feat, torch::Tensor thr,
                           torch::Tensor left, torch::Tensor right,
                           torch::Tensor leaf_index, torch::Tensor offsets,
                           torch::Tensor X,
                           c10::optional<torch::Tensor> cat_offset,
                           c10::optional<torch::Tensor> cat_words) {
  CHECK_DEV(X); CHECK_CONTIG(X);
  const long n = X.size(0);
  const long nf = X.size(1);
  const long n_trees = offsets.numel() - 1;
  auto out = torch::zeros({n, n_trees}, X.options().dtype(torch::kInt32));
  auto [co, cw] = cat_ptrs(cat_offset, cat_words);
  launch_predict_leaf(feat.data_ptr<int>(), thr.data_ptr<float>(),
                      left.data_ptr<int>(), right.data_ptr<int>(),
                      leaf_index.data_ptr<int>(), offsets.data_ptr<long>(),
                      X.data_ptr<float>(), n, (int)nf, out.data_ptr<int>(),
                      (int)n_trees, co, cw, cur_stream());
  return out;
}

// CSR-row scoring: the row is (indptr, col, xval) instead of X + row*nf.
// col must be strictly increasing within a row (CsrMatrix's precondition).
static long check_csr_rows(const torch::Tensor& indptr,
                           const torch::Tensor& col,
                           const torch::Tensor& xval) {
  CHECK_DEV(indptr); CHECK_CONTIG(indptr);
  CHECK_DEV(col); CHECK_CONTIG(col);
  CHECK_DEV(xval); CHECK_CONTIG(xval);
  TORCH_CHECK(indptr.dtype() == torch::kInt64, "indptr must be int64");
  TORCH_CHECK(col.dtype() == torch::kInt32, "col must be int32");
  TORCH_CHECK(xval.dtype() == torch::kFloat32, "xval must be float32");
  TORCH_CHECK(indptr.dim() == 1 && indptr.numel() >= 1,
              "indptr must hold n+1 row offsets");
  TORCH_CHECK(col.numel() == xval.numel(),
              "col and xval must have one entry per stored value");
  return indptr.numel() - 1;
}

torch::Tensor predict_forest_csr(torch::Tensor feat, torch::Tensor thr,
                                 torch::Tensor left, torch::Tensor right,
                                 torch::Tensor val, torch::Tensor offsets,
                                 torch::Tensor tw, torch::Tensor indptr,
                                 torch::Tensor col, torch::Tensor xval,
                                 long n_outputs, long t0, long t1,
                                 c10::optional<torch::Tensor> cat_offset,
                                 c10::optional<torch::Tensor> cat_words) {
  const long n = check_csr_rows(indptr, col, xval);
  CHECK_DEV(feat); CHECK_CONTIG(feat);
  CHECK_DEV(offsets); CHECK_CONTIG(offsets);
  TORCH_CHECK(offsets.dtype() == torch::kInt64, "offsets must be int64");
  TORCH_CHECK(n_outputs >= 1, "n_outputs must be positive");
  const long n_trees = offsets.numel() - 1;
  auto out = torch::zeros({n, n_outputs},
                          xval.options().dtype(torch::kFloat32));
  if (n == 0 || n_trees <= 0 || t1 <= t0) return out;
  TORCH_CHECK(t0 >= 0 && t1 <= n_trees, "tree window outside the forest");
  TORCH_CHECK(tw.numel() >= t1, "one weight per tree");
  auto [co, cw] = cat_ptrs(cat_offset, cat_words);
  launch_predict_forest_csr(
      feat.data_ptr<int>(), thr.data_ptr<float>(), left.data_ptr<int>(),
      right.data_ptr<int>(), val.data_ptr<float>(), offsets.data_ptr<long>(),
      tw.data_ptr<float>(), indptr.data_ptr<long>(), col.data_ptr<int>(),
      xval.data_ptr<float>(), n, out.data_ptr<float>(), (int)n_outputs,
      (int)t0, (int)t1, co, cw, cur_stream());
  return out;
}

torch::Tensor predict_leaf_csr(torch::Tensor feat, torch::Tensor thr,
                               torch::Tensor left, torch::Tensor right,
                               torch::Tensor leaf_index, torch::Tensor offsets,
                               torch::Tensor indptr, torch::Tensor col,
                               torch::Tensor xval,
                               c10::optional<torch::Tensor> cat_offset,
                               c10::optional<torch::Tensor> cat_words) {
  const long n = check_csr_rows(indptr, col, xval);
  CHECK_DEV(feat); CHECK_CONTIG(feat);
  CHECK_DEV(offsets); CHECK_CONTIG(offsets);
  TORCH_CHECK(offsets.dtype() == torch::kInt64, "offsets must be int64");
  const long n_trees = offsets.numel() - 1;
  auto out = torch::zeros({n, n_trees}, xval.options().dtype(torch::kInt32));
  if (n == 0 || n_trees <= 0) return out;
  auto [co, cw] = cat_ptrs(cat_offset, cat_words);
  launch_predict_leaf_csr(
      feat.data_ptr<int>(), thr.data_ptr<float>(), left.data_ptr<int>(),
      right.data_ptr<int>(), leaf_index.data_ptr<int>(),
      offsets.data_ptr<long>(), indptr.data_ptr<long>(), col.data_ptr<int>(),
      xval.data_ptr<float>(), n, out.data_ptr<int>(), (int)n_trees, co, cw,
      cur_stream());
  return out;
}

std::tuple<torch::Tensor, torch::Tensor> partition_rows(
    torch::Tensor binned_i4, torch::Tensor rows, long feature, long thr,
    long known_left) {
  CHECK_DEV(binned_i4); CHECK_CONTIG(binned_i4);
  CHECK_DEV(rows); CHECK_CONTIG(rows);
  TORCH_CHECK(rows.dtype() == torch::kInt32, "rows must be int32");
  const long m = rows.numel();
  auto out = torch::empty({m}, rows.options());
  auto scratch = torch::empty({4096}, rows.options());
  auto total = torch::zeros({1}, rows.options());
  if (m > 0) {
    launch_partition(binned_i4.data_ptr(), binned_i4.size(1),
                     rows.data_ptr<int>(), m, (int)feature, (int)thr,
                     out.data_ptr<int>(), scratch.data_ptr<int>(),
                     total.data_ptr<int>(), cur_stream());
  }
  // single-rank training already knows the exact left count from the split
  // stats (integer histogram counts) — skip the device→host sync entirely
  const long nl = known_left >= 0 ? known_left : total.item<int>();
  return {out.slice(0, 0, nl), out.slice(0, nl, m)};
}

torch::Tensor bin_matrix(torch::Tensor X, torch::Tensor ub, long n_bins) {
  CHECK_DEV(X); CHECK_CONTIG(X);
  CHECK_DEV(ub); CHECK_CONTIG(ub);
  // the bin is a uint8 and the kernel searches n_bins - 1 bounds per feature
  TORCH_CHECK(n_bins >= 2 && n_bins <= 256, "n_bins must be in 2..256");
  TORCH_CHECK(X.dim() == 2 && X.dtype() == torch::kFloat32,
              "X must be (n, nf) float32");
  TORCH_CHECK(X.device() == ub.device(), "ub must live where X lives");
  const long n = X.size(0);
  const long nf = X.size(1);
  TORCH_CHECK(ub.dim() == 2 && ub.dtype() == torch::kFloat32 &&
              ub.size(0) == nf && ub.size(1) == n_bins - 1,
              "ub must be (nf, n_bins - 1) float32");
  const long ngroups = (nf + 3) / 4;
  auto out = torch::zeros({ngroups, n, 4}, X.options().dtype(torch::kUInt8));
  launch_bin_matrix(X.data_ptr<float>(), ub.data_ptr<float>(), n, (int)nf,
                    (int)n_bins, (int)ngroups, out.data_ptr(), cur_stream());
  return out;
}

torch::Tensor split_scan(torch::Tensor hists, long n_bins, double l1,
                         double l2, double min_data, double min_hess,
                         double min_gain, long nf_real,
                         c10::optional<torch::Tensor> feat_mask) {
  // hists: (n_hists, nf_pad, n_bins, 3) — returns (n_hists, 6) on device:
  // {gain, feature, bin, GL, HL, CL}.  min_gain is not applied here: the
  // record carries the gain and the threshold is the caller's.
  (void)min_gain;
  CHECK_DEV(hists); CHECK_CONTIG(hists);
  TORCH_CHECK(hists.dim() == 4 && hists.dtype() == torch::kFloat32 &&
              hists.size(3) == 3,
              "hists must be (n_hists, nf_pad, n_bins, 3) float32");
  // one 256-thread block scans a feature: a bin per thread, 256 LDS slots
  TORCH_CHECK(n_bins >= 2 && n_bins <= 256, "n_bins must be in 2..256");
  TORCH_CHECK(hists.size(2) == n_bins, "n_bins must equal hists.size(2)");
  const long n_hists = hists.size(0);
  const long nf_pad = hists.size(1);
  TORCH_CHECK(nf_real > 0 && nf_real <= nf_pad,
              "nf_real must be in 1..nf_pad");
  auto scratch = torch::empty({n_hists, nf_pad, 6}, hists.options());
  auto out = torch::empty({n_hists, 6}, hists.options());
  const bool* mask_ptr = nullptr;
  if (feat_mask.has_value()) {
    TORCH_CHECK(feat_mask->device() == hists.device(),
                "feat_mask must live where hists lives");
    TORCH_CHECK(feat_mask->dtype() == torch::kBool, "feat_mask must be bool");
    TORCH_CHECK(feat_mask->is_contiguous() && feat_mask->numel() >= nf_pad,
                "feat_mask must be contiguous with at least nf_pad elements");
    mask_ptr = feat_mask->data_ptr<bool>();
  }
  if (n_hists == 0) return out;
  launch_split_scan(hists.data_ptr<float>(), (int)n_hists, nf_pad,
                    (int)n_bins, (float)l1, (float)l2, (float)min_data,
                    (float)min_hess, nf_real, mask_ptr,
                    scratch.data_ptr<float>(), out.data_ptr<float>(),
                    cur_stream());
  return out;
}

torch::Tensor vw_sgd_minibatch(torch::Tensor idx, torch::Tensor val,
                               torch::Tensor off, torch::Tensor label,
                               torch::Tensor w_tbl, torch::Tensor g_tbl,
                               double lr, double l2, double power_t,
                               long loss,
                               c10::optional<torch::Tensor> ex_weight,
                               c10::optional<torch::Tensor> s_tbl,
                               bool invariant) {
  CHECK_DEV(w_tbl); CHECK_CONTIG(w_tbl);
  const long n_ex = off.numel() - 1;
  auto preds = torch::zeros({n_ex}, w_tbl.options());
  const float* wptr = ex_weight.has_value() ? ex_weight->data_ptr<float>()
                                            : nullptr;
  float* sptr = s_tbl.has_value() ? s_tbl->data_ptr<float>() : nullptr;
  launch_vw_sgd(idx.data_ptr<int>(), val.data_ptr<float>(),
                off.data_ptr<long>(), label.data_ptr<float>(), wptr,
                w_tbl.data_ptr<float>(), g_tbl.data_ptr<float>(), sptr,
                (float)lr, (float)l2, (float)power_t, (int)loss,
                invariant ? 1 : 0, n_ex,
                preds.data_ptr<float>(), cur_stream());
  return preds;
}

torch::Tensor vw_predict(torch::Tensor idx, torch::Tensor val,
                         torch::Tensor off, torch::Tensor w_tbl) {
  CHECK_DEV(w_tbl); CHECK_CONTIG(w_tbl);
  const long n_ex = off.numel() - 1;
  auto out = torch::zeros({n_ex}, w_tbl.options());
  launch_vw_predict(idx.data_ptr<int>(), val.data_ptr<float>(),
                    off.data_ptr<long>(), w_tbl.data_ptr<float>(), n_ex,
                    out.data_ptr<float>(), cur_stream());
  return out;
}

torch::Tensor tree_shap(torch::Tensor feat, torch::Tensor thr,
                        torch::Tensor left, torch::Tensor right,
                        torch::Tensor val, torch::Tensor cnt,
                        torch::Tensor offsets, torch::Tensor X,
                        long n_outputs, long max_depth,
                        c10::optional<torch::Tensor> cat_offset,
                        c10::optional<torch::Tensor> cat_words) {
  CHECK_DEV(X); CHECK_CONTIG(X);
  const long n = X.size(0);
  const long nf = X.size(1);
  const long n_trees = offsets.numel() - 1;
  auto out = torch::zeros({n, n_outputs * (nf + 1)},
                          X.options().dtype(torch::kFloat32));
  auto [co, cw] = cat_ptrs(cat_offset, cat_words);
  launch_tree_shap(feat.data_ptr<int>(), thr.data_ptr<float>(),
                   left.data_ptr<int>(), right.data_ptr<int>(),
                   val.data_ptr<float>(), cnt.data_ptr<float>(),
                   offsets.data_ptr<long>(), co, cw, X.data_ptr<float>(), n,
                   (int)nf, (int)n_trees, (int)n_outputs, (int)max_depth,
                   out.data_ptr<float>(), cur_stream());
  return out;
}

// TreeSHAP over the CSR row window [row_begin, row_end) of the full indptr;
// compact result (rows, n_outputs, n_slots + 1), slot n_slots (the expected
// value) left zero for the caller.
torch::Tensor tree_shap_csr(torch::Tensor feat, torch::Tensor thr,
                            torch::Tensor left, torch::Tensor right,
                            torch::Tensor val, torch::Tensor cnt,
                            torch::Tensor offsets, torch::Tensor slot,
                            long n_slots, torch::Tensor indptr,
                            torch::Tensor col, torch::Tensor xval,
                            long n_outputs, long max_depth, long row_begin,
                            long row_end, long max_blocks,
                            c10::optional<torch::Tensor> cat_offset,
                            c10::optional<torch::Tensor> cat_words) {
  const long n = check_csr_rows(indptr, col, xval);
  CHECK_DEV(feat); CHECK_CONTIG(feat);
  CHECK_DEV(offsets); CHECK_CONTIG(offsets);
  CHECK_DEV(slot); CHECK_CONTIG(slot);
  CHECK_DEV(cnt); CHECK_CONTIG(cnt);
  TORCH_CHECK(offsets.dtype() == torch::kInt64, "offsets must be int64");
  TORCH_CHECK(slot.dtype() == torch::kInt32, "slot must be int32");
  TORCH_CHECK(slot.numel() == feat.numel() && cnt.numel() == feat.numel()
                  && val.numel() == feat.numel(),
              "slot, cnt and val must have one entry per node");
  TORCH_CHECK(n_outputs >= 1, "n_outputs must be positive");
  TORCH_CHECK(n_slots >= 0, "n_slots must not be negative");
  TORCH_CHECK(0 <= row_begin && row_begin <= row_end && row_end <= n,
              "row window outside the matrix");
  TORCH_CHECK(max_blocks >= 0, "max_blocks must not be negative");
  TORCH_CHECK(max_depth < 32, "trees of depth >= 32 need the CPU reference");
  const long n_trees = offsets.numel() - 1;
  auto out = torch::zeros({row_end - row_begin, n_outputs, n_slots + 1},
                          xval.options().dtype(torch::kFloat32));
  if (row_end == row_begin || n_trees <= 0) return out;
  auto [co, cw] = cat_ptrs(cat_offset, cat_words);
  launch_tree_shap_csr(
      feat.data_ptr<int>(), thr.data_ptr<float>(), left.data_ptr<int>(),
      right.data_ptr<int>(), val.data_ptr<float>(), cnt.data_ptr<float>(),
      offsets.data_ptr<long>(), slot.data_ptr<int>(), co, cw,
      indptr.data_ptr<long>(), col.data_ptr<int>(), xval.data_ptr<float>(),
      row_begin, row_end, (int)n_trees, (int)n_outputs, (int)n_slots,
      (int)max_depth, out.data_ptr<float>(), max_blocks, cur_stream());
  return out;
}

// --------------------------------------------------------------- sparse CSR
torch::Tensor csr_hist_fixed(torch::Tensor indptr, torch::Tensor col,
                             torch::Tensor binv, torch::Tensor gq,
                             torch::Tensor hq, torch::Tensor rows,
                             long nf, long n_bins) {
  CHECK_DEV(indptr); CHECK_CONTIG(indptr);
  CHECK_DEV(col); CHECK_CONTIG(col);
  CHECK_DEV(binv); CHECK_CONTIG(binv);
  CHECK_DEV(gq); CHECK_CONTIG(gq);
  CHECK_DEV(hq); CHECK_CONTIG(hq);
  CHECK_DEV(rows); CHECK_CONTIG(rows);
  TORCH_CHECK(indptr.dtype() == torch::kInt64, "indptr must be int64");
  TORCH_CHECK(col.dtype() == torch::kInt32, "col must be int32");
  TORCH_CHECK(binv.dtype() == torch::kUInt8, "binv must be uint8");
  TORCH_CHECK(gq.dtype() == torch::kInt64 && hq.dtype() == torch::kInt64,
              "gq/hq must be int64 fixed point");
  auto hist = torch::zeros({nf, n_bins, 3},
                           gq.options().dtype(torch::kInt64));
  launch_csr_hist_fixed(indptr.data_ptr<long>(), col.data_ptr<int>(),
                        binv.data_ptr<unsigned char>(),
                        (const long long*)gq.data_ptr<int64_t>(),
                        (const long long*)hq.data_ptr<int64_t>(),
                        rows.data_ptr<int>(), rows.numel(),
                        (long long*)hist.data_ptr<int64_t>(), (int)n_bins,
                        cur_stream());
  return hist;
}

// v2: wave-cooperative row chunks + in-kernel leaf totals
std::tuple<torch::Tensor, torch::Tensor> csr_hist_fixed_tot(
    torch::Tensor indptr, torch::Tensor col, torch::Tensor binv,
    torch::Tensor gq, torch::Tensor hq, torch::Tensor rows, long nf,
    long n_bins) {
  CHECK_DEV(indptr); CHECK_CONTIG(indptr);
  CHECK_DEV(col); CHECK_CONTIG(col);
  CHECK_DEV(binv); CHECK_CONTIG(binv);
  CHECK_DEV(gq); CHECK_CONTIG(gq);
  CHECK_DEV(hq); CHECK_CONTIG(hq);
  CHECK_DEV(rows); CHECK_CONTIG(rows);
  auto hist = torch::zeros({nf, n_bins, 3},
                           gq.options().dtype(torch::kInt64));
  auto tot = torch::zeros({3}, gq.options().dtype(torch::kInt64));
  if (nf <= 2048) {
    // small/medium nf: LDS-privatized feature chunks (redundant coalesced
    // reads, 9x-faster LDS atomics, one global flush per cell)
    launch_csr_hist_fixed_lds(indptr.data_ptr<long>(), col.data_ptr<int>(),
                              binv.data_ptr<unsigned char>(),
                              (const long long*)gq.data_ptr<int64_t>(),
                              (const long long*)hq.data_ptr<int64_t>(),
                              rows.data_ptr<int>(), rows.numel(),
                              (long long*)hist.data_ptr<int64_t>(),
                              (int)n_bins, (int)nf,
                              (long long*)tot.data_ptr<int64_t>(),
                              cur_stream());
  } else {
    // wide-nf: atomics spread across nf*n_bins cells — contention is low
    launch_csr_hist_fixed_v2(indptr.data_ptr<long>(), col.data_ptr<int>(),
                             binv.data_ptr<unsigned char>(),
                             (const long long*)gq.data_ptr<int64_t>(),
                             (const long long*)hq.data_ptr<int64_t>(),
                             rows.data_ptr<int>(), rows.numel(),
                             (long long*)hist.data_ptr<int64_t>(), (int)n_bins,
                             (long long*)tot.data_ptr<int64_t>(),
                             cur_stream());
  }
  return {hist, tot};
}

torch::Tensor csr_gather_bins(torch::Tensor indptr, torch::Tensor col,
                              torch::Tensor binv, torch::Tensor rows,
                              long feature, long zero_bin) {
  CHECK_DEV(indptr); CHECK_CONTIG(indptr);
  CHECK_DEV(col); CHECK_CONTIG(col);
  CHECK_DEV(binv); CHECK_CONTIG(binv);
  CHECK_DEV(rows); CHECK_CONTIG(rows);
  auto out = torch::empty({rows.numel()},
                          rows.options().dtype(torch::kInt32));
  launch_csr_gather_bin(indptr.data_ptr<long>(), col.data_ptr<int>(),
                        binv.data_ptr<unsigned char>(), rows.data_ptr<int>(),
                        rows.numel(), (int)feature, (int)zero_bin,
                        out.data_ptr<int>(), cur_stream());
  return out;
}

std::tuple<torch::Tensor, torch::Tensor> csr_partition_rows(
    torch::Tensor indptr, torch::Tensor col, torch::Tensor binv,
    torch::Tensor rows, long feature, long zero_bin, long thr,
    long known_left) {
  CHECK_DEV(indptr); CHECK_CONTIG(indptr);
  CHECK_DEV(col); CHECK_CONTIG(col);
  CHECK_DEV(binv); CHECK_CONTIG(binv);
  CHECK_DEV(rows); CHECK_CONTIG(rows);
  const long m = rows.numel();
  auto out = torch::empty({m}, rows.options());
  auto pred = torch::empty({m}, rows.options().dtype(torch::kUInt8));
  auto scratch = torch::empty({4096}, rows.options());
  auto total = torch::zeros({1}, rows.options());
  if (m > 0) {
    launch_csr_partition(indptr.data_ptr<long>(), col.data_ptr<int>(),
                         binv.data_ptr<unsigned char>(), rows.data_ptr<int>(),
                         m, (int)feature, (int)zero_bin, (int)thr, nullptr,
                         pred.data_ptr<unsigned char>(),
                         out.data_ptr<int>(), scratch.data_ptr<int>(),
                         total.data_ptr<int>(), cur_stream());
  }
  const long nl = known_left >= 0 ? known_left : total.item<int>();
  return {out.slice(0, 0, nl), out.slice(0, nl, m)};
}

// ------------------------------------------------------------------- images
// JPEG reconstruction (dequant + IDCT + colour + crop) of a whole batch in
// one launch, written into `out` in place.  The descriptors must already
// have passed ops/backend.py::check_jpeg_descriptors — this only checks that
// the tensors are what the kernel's pointer types say they are.
void jpeg_reconstruct(torch::Tensor coef, torch::Tensor qt,
                      torch::Tensor img_desc, torch::Tensor comp_desc,
                      torch::Tensor work_off, long n_items,
                      torch::Tensor out) {
  CHECK_DEV(coef); CHECK_CONTIG(coef);
  CHECK_DEV(qt); CHECK_CONTIG(qt);
  CHECK_DEV(img_desc); CHECK_CONTIG(img_desc);
  CHECK_DEV(comp_desc); CHECK_CONTIG(comp_desc);
  CHECK_DEV(work_off); CHECK_CONTIG(work_off);
  CHECK_DEV(out); CHECK_CONTIG(out);
  TORCH_CHECK(coef.dtype() == torch::kInt16, "coef must be int16");
  TORCH_CHECK(qt.dtype() == torch::kUInt16, "qt must be uint16");
  TORCH_CHECK(img_desc.dtype() == torch::kInt64 &&
              comp_desc.dtype() == torch::kInt64 &&
              work_off.dtype() == torch::kInt64,
              "descriptors must be int64");
  TORCH_CHECK(out.dtype() == torch::kUInt8, "out must be uint8");
  const long n_img = img_desc.size(0);
  TORCH_CHECK(img_desc.numel() == n_img * 4 &&
              comp_desc.numel() == n_img * 12 &&
              work_off.numel() == n_img + 1 &&
              qt.numel() == n_img * 4 * 64,
              "descriptor shapes do not agree on the batch size");
  TORCH_CHECK(n_img < (1L << 31) && n_items >= 0 && n_items < (1L << 31),
              "batch too large for one launch");
  TORCH_CHECK(((uintptr_t)out.data_ptr() & 3) == 0,
              "out must be 4-byte aligned");
  if (n_img == 0 || n_items == 0) return;
  launch_jpeg_reconstruct(
      (const short*)coef.data_ptr<int16_t>(),
      (const unsigned short*)qt.data_ptr(), img_desc.data_ptr<long>(),
      comp_desc.data_ptr<long>(), work_off.data_ptr<long>(), (int)n_img,
      n_items, out.data_ptr<uint8_t>(), cur_stream());
}

// Fused crop / flip / resize / channel map / pointwise ops / layout of a
// ragged image batch in one launch (image_preprocess_k), written into `out`
// in place.  The descriptors must already have passed
// ops/backend.py::check_image_descriptors; this checks the tensors against
// the kernel's pointer types, and the kernel range-checks every index again.
void image_preprocess(torch::Tensor src, torch::Tensor idesc,
                      torch::Tensor fdesc, torch::Tensor work_off,
                      long n_items, torch::Tensor out) {
  CHECK_DEV(src); CHECK_CONTIG(src);
  CHECK_DEV(idesc); CHECK_CONTIG(idesc);
  CHECK_DEV(fdesc); CHECK_CONTIG(fdesc);
  CHECK_DEV(work_off); CHECK_CONTIG(work_off);
  CHECK_DEV(out); CHECK_CONTIG(out);
  TORCH_CHECK(src.dtype() == torch::kUInt8 || src.dtype() == torch::kFloat32,
              "src must be uint8 or float32");
  TORCH_CHECK(out.dtype() == torch::kUInt8 || out.dtype() == torch::kFloat32,
              "out must be uint8 or float32");
  TORCH_CHECK(idesc.dtype() == torch::kInt64 &&
              work_off.dtype() == torch::kInt64,
              "idesc and work_off must be int64");
  TORCH_CHECK(fdesc.dtype() == torch::kFloat32, "fdesc must be float32");
  TORCH_CHECK(src.get_device() == out.get_device() &&
              idesc.get_device() == out.get_device() &&
              fdesc.get_device() == out.get_device() &&
              work_off.get_device() == out.get_device(),
              "all tensors must share one device");
  const long n_img = idesc.dim() == 2 ? idesc.size(0) : -1;
  TORCH_CHECK(n_img >= 0 && idesc.numel() == n_img * 24 &&
              fdesc.numel() == n_img * 34 && work_off.numel() == n_img + 1,
              "descriptor shapes do not agree on the batch size");
  TORCH_CHECK(n_img < (1L << 31) && n_items >= 0 && n_items < (1L << 31),
              "batch too large for one launch");
  if (n_img == 0 || n_items == 0) return;
  launch_image_preprocess(
      src.data_ptr(), src.numel(), src.dtype() == torch::kFloat32,
      idesc.data_ptr<long>(), fdesc.data_ptr<float>(),
      work_off.data_ptr<long>(), (int)n_img, n_items, out.data_ptr(),
      out.numel(), out.dtype() == torch::kFloat32, cur_stream());
}

// ------------------------------------------------------------------ ranking
// Shared checks of the per-fit group table (rank_kernels.hip): offsets
// (G+1) int64, gid (n) int32.  Their contents are validated on the host when
// they are built (models/gbdt/ranking.py); the kernels clamp what is left.
static void check_group_table(const torch::Tensor& offsets,
                              const torch::Tensor& gid, long n) {
  CHECK_DEV(offsets); CHECK_CONTIG(offsets);
  CHECK_DEV(gid); CHECK_CONTIG(gid);
  TORCH_CHECK(offsets.dtype() == torch::kInt64, "offsets must be int64");
  TORCH_CHECK(gid.dtype() == torch::kInt32, "gid must be int32");
  TORCH_CHECK(offsets.dim() == 1 && offsets.numel() >= 1,
              "offsets must be a (G+1) vector");
  TORCH_CHECK(offsets.numel() - 1 < (1L << 31), "too many groups");
  TORCH_CHECK(gid.dim() == 1 && gid.numel() == n,
              "gid must have one entry per document");
  TORCH_CHECK(n < (1L << 31), "too many documents for int32 ranks");
}

std::tuple<torch::Tensor, torch::Tensor> group_rank(
    torch::Tensor score, torch::Tensor offsets, torch::Tensor gid,
    torch::Tensor label, torch::Tensor gain, torch::Tensor disc_tbl) {
  CHECK_DEV(score); CHECK_CONTIG(score);
  CHECK_DEV(label); CHECK_CONTIG(label);
  CHECK_DEV(gain); CHECK_CONTIG(gain);
  CHECK_DEV(disc_tbl); CHECK_CONTIG(disc_tbl);
  TORCH_CHECK(score.dtype() == torch::kFloat32 &&
              label.dtype() == torch::kFloat32 &&
              gain.dtype() == torch::kFloat32 &&
              disc_tbl.dtype() == torch::kFloat32,
              "score, label, gain and disc_tbl must be float32");
  TORCH_CHECK(score.dim() == 1, "score must be a vector");
  const long n = score.numel();
  check_group_table(offsets, gid, n);
  TORCH_CHECK(label.numel() == n && gain.numel() == n,
              "label and gain must have one entry per document");
  auto rank = torch::empty({n}, score.options().dtype(torch::kInt32));
  auto rec = torch::empty({n, 4}, score.options());
  if (n == 0) return {rank, rec};
  launch_group_rank(score.data_ptr<float>(), offsets.data_ptr<long>(),
                    gid.data_ptr<int>(), label.data_ptr<float>(),
                    gain.data_ptr<float>(), disc_tbl.data_ptr<float>(), n,
                    (int)(offsets.numel() - 1), disc_tbl.numel(),
                    rank.data_ptr<int>(), rec.data_ptr(), cur_stream());
  return {rank, rec};
}

std::tuple<torch::Tensor, torch::Tensor> lambdarank_grad(
    torch::Tensor records, torch::Tensor offsets, torch::Tensor gid,
    torch::Tensor inv_idcg, double sigma) {
  CHECK_DEV(records); CHECK_CONTIG(records);
  CHECK_DEV(inv_idcg); CHECK_CONTIG(inv_idcg);
  TORCH_CHECK(records.dtype() == torch::kFloat32 &&
              inv_idcg.dtype() == torch::kFloat32,
              "records and inv_idcg must be float32");
  TORCH_CHECK(records.dim() == 2 && records.size(1) == 4,
              "records must be (n, 4)");
  const long n = records.size(0);
  check_group_table(offsets, gid, n);
  TORCH_CHECK(inv_idcg.numel() == offsets.numel() - 1,
              "inv_idcg must have one entry per group");
  auto g = torch::empty({n}, records.options());
  auto h = torch::empty({n}, records.options());
  if (n == 0) return {g, h};
  TORCH_CHECK(((uintptr_t)records.data_ptr() & 15) == 0,
              "records must be 16-byte aligned");
  launch_lambdarank_grad(records.data_ptr(), offsets.data_ptr<long>(),
                         gid.data_ptr<int>(), inv_idcg.data_ptr<float>(),
                         (float)sigma, n, (int)(offsets.numel() - 1),
                         g.data_ptr<float>(), h.data_ptr<float>(),
                         cur_stream());
  return {g, h};
}

// ------------------------------------------------------ nearest neighbours
// knn_kernels.hip.  The contents of label_ids are range-checked by the caller
// (ops/backend.py) and clamped again in the kernel.
static const int kKnnMaxK = 64;
static const int kKnnMaxSplits = 64;

std::tuple<torch::Tensor, torch::Tensor> knn_topk(
    torch::Tensor Q, torch::Tensor X, torch::Tensor xsq, long k,
    c10::optional<torch::Tensor> label_ids,
    c10::optional<torch::Tensor> allow_bits, long splits) {
  CHECK_DEV(Q); CHECK_CONTIG(Q);
  CHECK_DEV(X); CHECK_CONTIG(X);
  CHECK_DEV(xsq); CHECK_CONTIG(xsq);
  TORCH_CHECK(Q.dtype() == torch::kFloat32 && X.dtype() == torch::kFloat32 &&
              xsq.dtype() == torch::kFloat32,
              "Q, X and xsq must be float32");
  TORCH_CHECK(Q.dim() == 2 && X.dim() == 2 && Q.size(1) == X.size(1),
              "Q (n_q, d) and X (n, d) must agree on d");
  const long n_q = Q.size(0), n = X.size(0), d = X.size(1);
  TORCH_CHECK(xsq.dim() == 1 && xsq.numel() == n, "xsq must be (n,)");
  TORCH_CHECK(k >= 1 && k <= kKnnMaxK, "k out of range");
  TORCH_CHECK(n < (1L << 31) && d >= 1 && d < (1L << 24),
              "index too large");
  TORCH_CHECK(splits >= 0 && splits <= kKnnMaxSplits, "splits out of range");
  TORCH_CHECK(label_ids.has_value() == allow_bits.has_value(),
              "label_ids and allow_bits go together");
  const int* lid = nullptr;
  const unsigned* bits = nullptr;
  int W = 0;
  if (label_ids.has_value()) {
    const auto& l = *label_ids;
    const auto& b = *allow_bits;
    CHECK_DEV(l); CHECK_CONTIG(l);
    CHECK_DEV(b); CHECK_CONTIG(b);
    TORCH_CHECK(l.dtype() == torch::kInt32 && l.dim() == 1 && l.numel() == n,
                "label_ids must be (n,) int32");
    TORCH_CHECK(b.dtype() == torch::kInt32 && b.dim() == 2 &&
                b.size(0) == n_q && b.size(1) >= 1 && b.size(1) < (1L << 20),
                "allow_bits must be (n_q, W) int32");
    lid = l.data_ptr<int>();
    bits = (const unsigned*)b.data_ptr<int>();
    W = (int)b.size(1);
  }
  auto d2 = torch::full({n_q, k}, std::numeric_limits<float>::infinity(),
                        Q.options());
  auto idx = torch::full({n_q, k}, -1, Q.options().dtype(torch::kInt32));
  if (n_q == 0 || n == 0) return {d2, idx};
  const int sp = knn_choose_splits(n_q, n, (int)k, (int)splits);
  const long q_tiles = (n_q + 127) / 128;
  TORCH_CHECK(n_q < (1L << 31) && q_tiles * sp < (1L << 31),
              "too many queries for one launch");
  auto qsq = (Q * Q).sum(1);
  auto part_s = torch::empty({n_q, sp, k}, Q.options());
  auto part_i = torch::empty({n_q, sp, k}, idx.options());
  const int err = launch_knn_topk(
      Q.data_ptr<float>(), X.data_ptr<float>(), xsq.data_ptr<float>(),
      qsq.data_ptr<float>(), lid, bits, n_q, n, (int)d, (int)k, W, sp,
      part_s.data_ptr<float>(), part_i.data_ptr<int>(), d2.data_ptr<float>(),
      idx.data_ptr<int>(), cur_stream());
  TORCH_CHECK(err == 0, "knn_topk launch failed: ",
              hipGetErrorString((hipError_t)err));
  return {d2, idx};
}

// ------------------------------------------------------------ recommendation
// sar_kernels.hip.  CSR structure (sorted columns, indptr monotone) is checked
// by the caller (ops/backend.py); shapes, dtypes and ranges of scalars here.
static const int kSarMaxK = 128;
static const int kSarMaxTile = 16384;

static void sar_check_csr(const torch::Tensor& indptr, const torch::Tensor& col,
                          const torch::Tensor* val, const char* name) {
  CHECK_DEV(indptr); CHECK_CONTIG(indptr);
  CHECK_DEV(col); CHECK_CONTIG(col);
  TORCH_CHECK(indptr.dtype() == torch::kInt64 && indptr.dim() == 1 &&
              indptr.numel() >= 1, name, " indptr must be (rows + 1,) int64");
  TORCH_CHECK(col.dtype() == torch::kInt32 && col.dim() == 1, name,
              " col must be int32");
  if (val != nullptr) {
    CHECK_DEV((*val)); CHECK_CONTIG((*val));
    TORCH_CHECK(val->dtype() == torch::kFloat32 && val->dim() == 1 &&
                val->numel() == col.numel(), name,
                " val must be float32, one per column");
  }
}

static int sar_tile(long tile, long n_items, int which) {
  TORCH_CHECK(tile >= 0 && tile <= kSarMaxTile && tile % 64 == 0,
              "tile must be 0 or a multiple of 64 up to ", kSarMaxTile);
  return tile == 0 ? sar_default_tile(n_items, which) : (int)tile;
}

// Sparse Bt.B with threshold and similarity fused: (indptr, col, val) of S.
// sim: 0 cooccurrence, 1 jaccard, 2 lift.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> sar_cooccurrence(
    torch::Tensor b_indptr, torch::Tensor b_col, torch::Tensor bt_indptr,
    torch::Tensor bt_col, long threshold, long sim, long tile) {
  sar_check_csr(b_indptr, b_col, nullptr, "B");
  sar_check_csr(bt_indptr, bt_col, nullptr, "Bt");
  const long n_users = b_indptr.numel() - 1, n_items = bt_indptr.numel() - 1;
  TORCH_CHECK(n_users < (1L << 31) && n_items < (1L << 31),
              "too many users or items");
  TORCH_CHECK(sim >= 0 && sim <= 2, "unknown similarity function");
  TORCH_CHECK(threshold >= 1 && threshold < (1L << 31), "threshold out of range");
  const int T = sar_tile(tile, n_items, 0);
  const long n_tiles = (n_items + T - 1) / T;
  TORCH_CHECK(n_tiles <= 65535, "too many item tiles: use a wider tile");
  auto iopt = b_col.options();
  if (n_items == 0)
    return {torch::zeros({1}, b_indptr.options()), torch::empty({0}, iopt),
            torch::empty({0}, iopt.dtype(torch::kFloat32))};
  auto counts = torch::empty({n_items * n_tiles}, iopt);
  int err = launch_sar_cooc_count(
      bt_indptr.data_ptr<long>(), bt_col.data_ptr<int>(),
      b_indptr.data_ptr<long>(), b_col.data_ptr<int>(), (int)n_users,
      (int)n_items, T, (unsigned)threshold, counts.data_ptr<int>(),
      cur_stream());
  TORCH_CHECK(err == 0, "sar_cooc_count launch failed: ",
              hipGetErrorString((hipError_t)err));
  auto incl = counts.cumsum(0, torch::kInt64);
  auto offsets = (incl - counts).contiguous();
  const long nnz = incl[-1].item<long>();
  auto indptr = torch::cat({offsets.slice(0, 0, n_items * n_tiles, n_tiles),
                            incl.slice(0, n_items * n_tiles - 1)});
  auto col = torch::empty({nnz}, iopt);
  auto val = torch::empty({nnz}, iopt.dtype(torch::kFloat32));
  if (nnz > 0) {
    err = launch_sar_cooc_fill(
        bt_indptr.data_ptr<long>(), bt_col.data_ptr<int>(),
        b_indptr.data_ptr<long>(), b_col.data_ptr<int>(), (int)n_users,
        (int)n_items, T, (unsigned)threshold, (int)sim,
        offsets.data_ptr<long>(), nnz, col.data_ptr<int>(),
        val.data_ptr<float>(), cur_stream());
    TORCH_CHECK(err == 0, "sar_cooc_fill launch failed: ",
                hipGetErrorString((hipError_t)err));
  }
  return {indptr.contiguous(), col, val};
}

// Top-k items per requested user: (items (n, k) int32, scores (n, k) float32)
std::tuple<torch::Tensor, torch::Tensor> sar_recommend(
    torch::Tensor a_indptr, torch::Tensor a_col, torch::Tensor a_val,
    torch::Tensor s_indptr, torch::Tensor s_col, torch::Tensor s_val,
    c10::optional<torch::Tensor> users, long k, bool remove_seen, long tile) {
  sar_check_csr(a_indptr, a_col, &a_val, "affinity");
  sar_check_csr(s_indptr, s_col, &s_val, "similarity");
  const long n_users = a_indptr.numel() - 1, n_items = s_indptr.numel() - 1;
  TORCH_CHECK(n_users < (1L << 31) && n_items < (1L << 31),
              "too many users or items");
  TORCH_CHECK(k >= 1 && k <= kSarMaxK, "k out of range");
  const int T = sar_tile(tile, n_items, 1);
  const int* up = nullptr;
  long n = n_users;
  if (users.has_value()) {
    const auto& u = *users;
    CHECK_DEV(u); CHECK_CONTIG(u);
    TORCH_CHECK(u.dtype() == torch::kInt32 && u.dim() == 1,
                "users must be (n,) int32");
    up = u.data_ptr<int>();
    n = u.numel();
  }
  TORCH_CHECK(n < (1L << 31), "too many users for one launch");
  auto scores = torch::empty({n, k}, a_val.options());
  auto items = torch::empty({n, k}, a_col.options());
  if (n == 0) return {items, scores};
  const int err = launch_sar_recommend(
      a_indptr.data_ptr<long>(), a_col.data_ptr<int>(),
      a_val.data_ptr<float>(), s_indptr.data_ptr<long>(),
      s_col.data_ptr<int>(), s_val.data_ptr<float>(), up, n, (int)n_users,
      (int)n_items, T, (int)k, remove_seen ? 1 : 0, scores.data_ptr<float>(),
      items.data_ptr<int>(), cur_stream());
  TORCH_CHECK(err == 0, "sar_recommend launch failed: ",
              hipGetErrorString((hipError_t)err));
  return {items, scores};
}

torch::Tensor sar_score_pairs(
    torch::Tensor a_indptr, torch::Tensor a_col, torch::Tensor a_val,
    torch::Tensor s_indptr, torch::Tensor s_col, torch::Tensor s_val,
    torch::Tensor users, torch::Tensor items) {
  sar_check_csr(a_indptr, a_col, &a_val, "affinity");
  sar_check_csr(s_indptr, s_col, &s_val, "similarity");
  CHECK_DEV(users); CHECK_CONTIG(users);
  CHECK_DEV(items); CHECK_CONTIG(items);
  TORCH_CHECK(users.dtype() == torch::kInt32 && items.dtype() == torch::kInt32 &&
              users.dim() == 1 && items.dim() == 1 &&
              users.numel() == items.numel(),
              "users and items must be (n,) int32");
  const long n_users = a_indptr.numel() - 1, n_items = s_indptr.numel() - 1;
  TORCH_CHECK(n_users < (1L << 31) && n_items < (1L << 31),
              "too many users or items");
  const long n = users.numel();
  TORCH_CHECK(n < (1L << 39), "too many pairs for one launch");
  auto out = torch::empty({n}, a_val.options());
  if (n == 0) return out;
  const int err = launch_sar_score_pairs(
      a_indptr.data_ptr<long>(), a_col.data_ptr<int>(),
      a_val.data_ptr<float>(), s_indptr.data_ptr<long>(),
      s_col.data_ptr<int>(), s_val.data_ptr<float>(), users.data_ptr<int>(),
      items.data_ptr<int>(), n, (int)n_users, (int)n_items,
      out.data_ptr<float>(), cur_stream());
  TORCH_CHECK(err == 0, "sar_score_pairs launch failed: ",
              hipGetErrorString((hipError_t)err));
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("hist_build", &hist_build, "per-leaf (feature,bin) grad/hess/count histogram");
  m.def("hist_build_fixed_pair", &hist_build_fixed_pair,
        "fixed-point histogram over paired (8-feature) planes");
  m.def("hist_build_fixed", &hist_build_fixed,
        "fixed-point u64 histogram (fast LDS integer atomics)");
  m.def("predict_forest", &predict_forest, "GBDT ensemble raw scores");
  m.def("predict_leaf", &predict_leaf, "GBDT per-tree leaf indices");
  m.def("predict_forest_csr", &predict_forest_csr,
        "GBDT ensemble raw scores over CSR rows (no densify)");
  m.def("predict_leaf_csr", &predict_leaf_csr,
        "GBDT per-tree leaf indices over CSR rows (no densify)");
  m.def("bin_matrix", &bin_matrix, "quantile binning to interleaved uint8");
  m.def("split_scan", &split_scan, "fused best-split over sibling histograms");
  m.def("partition_rows", &partition_rows,
        "stable ordered row partition, single sync");
  m.def("vw_sgd_minibatch", &vw_sgd_minibatch, "adaptive sparse SGD minibatch");
  m.def("vw_predict", &vw_predict, "sparse linear predict");
  m.def("tree_shap", &tree_shap, "path-dependent TreeSHAP contributions");
  m.def("tree_shap_csr", &tree_shap_csr,
        "TreeSHAP over CSR rows, compact per-used-feature contributions");
  m.def("csr_hist_fixed", &csr_hist_fixed,
        "fixed-point histogram over stored CSR entries");
  m.def("csr_gather_bins", &csr_gather_bins,
        "per-row bin of one feature from CSR (missing -> zero bin)");
  m.def("csr_partition_rows", &csr_partition_rows,
        "fused CSR leaf partition (binary-search predicate, single sync)");
  m.def("csr_hist_fixed_tot", &csr_hist_fixed_tot,
        "wave-cooperative CSR histogram + in-kernel leaf totals");
  m.def("jpeg_reconstruct", &jpeg_reconstruct,
        "batched JPEG dequant + IDCT + colour conversion into a uint8 buffer");
  m.def("image_preprocess", &image_preprocess,
        "fused crop/flip/resize/colour/threshold/normalize of a ragged batch");
  m.def("image_work_items", &image_work_items,
        "work items (64 x 8 output tiles) image_preprocess_k spends on Ho x Wo");
  m.def("group_rank", &group_rank,
        "stable descending in-group ranks + per-document rank records");
  m.def("lambdarank_grad", &lambdarank_grad,
        "lambdarank gradients and hessians over all query groups");
  m.def("knn_topk", &knn_topk,
        "fused exact k-nearest-neighbour search with optional label bitsets");
  m.attr("KNN_MAX_K") = kKnnMaxK;
  m.attr("KNN_MAX_SPLITS") = kKnnMaxSplits;
  m.def("sar_cooccurrence", &sar_cooccurrence,
        "sparse item-item co-occurrence with threshold and similarity fused");
  m.def("sar_recommend", &sar_recommend,
        "fused SAR scoring + exact top-k per user over CSR affinity/similarity");
  m.def("sar_score_pairs", &sar_score_pairs,
        "SAR score of (user, item) pairs, bit-equal to sar_recommend's");
  m.def("sar_default_tile", &sar_default_tile,
        "tile the SAR launchers pick (which: 0 co-occurrence, 1 recommend)");
  m.attr("SAR_MAX_K") = kSarMaxK;
  m.attr("SAR_MAX_TILE") = kSarMaxTile;
}
