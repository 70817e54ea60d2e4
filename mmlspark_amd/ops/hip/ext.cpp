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
void launch_hist_build_fixed_pair(const void*, long, const int*, long,
                                  const float*, const float*, long long*, int,
                                  int, int, double, double, hipStream_t);
void launch_partition(const void*, long, const int*, long, int, int, int*,
                      int*, int*, hipStream_t);
void launch_split_scan(const float*, int, long, int, float, float, float,
                       float, long, const bool*, float*, float*, hipStream_t);
void launch_vw_sgd(const int*, const float*, const long*, const float*,
                   const float*, float*, float*, float*, float, float, float,
                   int, int, long, float*, hipStream_t);
void launch_vw_predict(const int*, const float*, const long*, const float*,
                       long, float*, hipStream_t);
int vw_interact_window();
int vw_interact_max_pairs();
int launch_vw_sgd_interact(const int*, const float*, const long*, const int*,
                           int, const int*, const int*, int, int,
                           const float*, const float*, float*, float*, float*,
                           float, float, float, int, int, long, float*,
                           hipStream_t);
int launch_vw_predict_interact(const int*, const float*, const long*,
                               const int*, int, const int*, const int*, int,
                               int, const float*, long, float*, hipStream_t);
void launch_tree_shap(const int*, const float*, const int*, const int*,
                      const float*, const float*, const long*, const int*,
                      const unsigned*, const float*, long, int, int, int, int,
                      float*, hipStream_t);
void launch_tree_shap_csr(const int*, const float*, const int*, const int*,
                          const float*, const float*, const long*, const int*,
                          const int*, const unsigned*, const long*, const int*,
                          const float*, long, long, int, int, int, int, float*,
                          long, hipStream_t);
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
int explain_draw_splits(long, long, int);
int launch_coalition_values(const int*, const float*, const int*, const int*,
                            const float*, const long*, const float*,
                            const int*, const unsigned*, long, int, int, int,
                            const float*, long, const float*, int, int,
                            const unsigned*, int, int, const int*, int,
                            const float*, int, float, const int*, int, int,
                            double*, double*, hipStream_t);
int als_heavy_degree();
int als_gram_blocks(long);
int launch_als_gram(const float*, long, int, float*, float*, hipStream_t);
int launch_als_solve_rows(const long*, const int*, const float*, const float*,
                          const float*, int, int, float, float, int, long,
                          float*, hipStream_t);
int launch_als_solve_heavy(const long*, const int*, const float*, const float*,
                           const float*, const int*, int, int, float, float,
                           int, float*, hipStream_t);
int launch_als_score_pairs(const float*, const float*, const int*, const int*,
                           const int*, const long*, const long*, const double*,
                           const double*, int, int, long, float*, hipStream_t);
int launch_slic_segment(const unsigned char*, long, const long*, const long*,
                        int, long, int, long, float*, unsigned long long*,
                        int*, long, float, int, int, hipStream_t);
int launch_masked_image_batch(const unsigned char*, int, int, int, const int*,
                              const unsigned*, int, int, int, int, int,
                              const float*, float*, hipStream_t);
int iforest_max_sub();
int iforest_staged(int, int);
int launch_iforest_build(const float*, long, int, int, int, int, int,
                         unsigned long long, int*, int*, float*, int*, int*,
                         int*, int*, int*, hipStream_t);
int launch_iforest_compact(const int*, const float*, const int*, const int*,
                           const int*, const int*, const long*, int, int,
                           int*, float*, int*, int*, int*, int*, hipStream_t);
int lime_fit_max_features();
int lime_fit_max_outputs();
long lime_fit_scratch_doubles(int);
int launch_lime_fit(const int*, const double*, int, int, int, int, double,
                    double, int, double, double*, double*, double*, double*,
                    int*, hipStream_t);
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
                               (long long*)hist.data_ptr<int64_t>(),
                               (int)n_bins, (int)npairs, (int)tail_bytes,
                               scale_g, scale_h, cur_stream());
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

// vw_interact_kernels.hip: the compact namespace batch.  idx/val hold each
// column's raw entries once; ns_off (n_ex, n_cols + 1) bounds them; pairs
// (n_pairs, 2) names the columns to cross.  Returns n_ex, n_cols, n_pairs.
static std::tuple<long, int, int> check_vw_interact(
    const torch::Tensor& idx, const torch::Tensor& val,
    const torch::Tensor& ns_off, const torch::Tensor& col_seed,
    const torch::Tensor& pairs, const torch::Tensor& pair_seed, long bits,
    const torch::Tensor& w_tbl) {
  CHECK_DEV(idx); CHECK_CONTIG(idx);
  CHECK_DEV(val); CHECK_CONTIG(val);
  CHECK_DEV(ns_off); CHECK_CONTIG(ns_off);
  CHECK_DEV(col_seed); CHECK_CONTIG(col_seed);
  CHECK_DEV(pairs); CHECK_CONTIG(pairs);
  CHECK_DEV(pair_seed); CHECK_CONTIG(pair_seed);
  CHECK_DEV(w_tbl); CHECK_CONTIG(w_tbl);
  TORCH_CHECK(idx.dtype() == torch::kInt32 && val.dtype() == torch::kFloat32
              && idx.dim() == 1 && idx.numel() == val.numel(),
              "idx int32 and val float32 of one length");
  TORCH_CHECK(col_seed.dtype() == torch::kInt32 && col_seed.dim() == 1,
              "col_seed must be int32 (n_cols)");
  const long n_cols = col_seed.numel();
  TORCH_CHECK(ns_off.dtype() == torch::kInt64 && ns_off.dim() == 2
              && ns_off.size(1) == n_cols + 1,
              "ns_off must be int64 (n_ex, n_cols + 1)");
  TORCH_CHECK(pairs.dtype() == torch::kInt32 && pairs.dim() == 2
              && pairs.size(1) == 2, "pairs must be int32 (n_pairs, 2)");
  TORCH_CHECK(pair_seed.dtype() == torch::kInt32 && pair_seed.dim() == 1
              && pair_seed.numel() == pairs.size(0),
              "pair_seed must be int32 (n_pairs)");
  TORCH_CHECK(pairs.size(0) <= vw_interact_max_pairs(), "at most ",
              vw_interact_max_pairs(), " pairs");
  TORCH_CHECK(n_cols < (1L << 20), "too many columns");
  TORCH_CHECK(bits >= 1 && bits <= 30, "bits must be in [1, 30]");
  TORCH_CHECK(w_tbl.dtype() == torch::kFloat32
              && w_tbl.numel() >= (1L << bits),
              "the weight table must hold 2^bits float32");
  return {ns_off.size(0), (int)n_cols, (int)pairs.size(0)};
}

torch::Tensor vw_sgd_minibatch_interact(
    torch::Tensor idx, torch::Tensor val, torch::Tensor ns_off,
    torch::Tensor col_seed, torch::Tensor pairs, torch::Tensor pair_seed,
    long bits, torch::Tensor label, torch::Tensor w_tbl, torch::Tensor g_tbl,
    double lr, double l2, double power_t, long loss,
    c10::optional<torch::Tensor> ex_weight,
    c10::optional<torch::Tensor> s_tbl, bool invariant) {
  auto [n_ex, n_cols, n_pairs] = check_vw_interact(
      idx, val, ns_off, col_seed, pairs, pair_seed, bits, w_tbl);
  CHECK_DEV(g_tbl); CHECK_CONTIG(g_tbl);
  CHECK_DEV(label); CHECK_CONTIG(label);
  TORCH_CHECK(g_tbl.dtype() == torch::kFloat32
              && g_tbl.numel() == w_tbl.numel(), "g_tbl must match w_tbl");
  TORCH_CHECK(label.dtype() == torch::kFloat32 && label.numel() == n_ex,
              "one float32 label per example");
  TORCH_CHECK(loss >= 0 && loss <= 2, "loss must be 0, 1 or 2");
  const float* wptr = nullptr;
  if (ex_weight.has_value()) {
    CHECK_DEV((*ex_weight)); CHECK_CONTIG((*ex_weight));
    TORCH_CHECK(ex_weight->dtype() == torch::kFloat32
                && ex_weight->numel() == n_ex,
                "one float32 importance weight per example");
    wptr = ex_weight->data_ptr<float>();
  }
  float* sptr = nullptr;
  if (s_tbl.has_value()) {
    CHECK_DEV((*s_tbl)); CHECK_CONTIG((*s_tbl));
    TORCH_CHECK(s_tbl->dtype() == torch::kFloat32
                && s_tbl->numel() == w_tbl.numel(),
                "s_tbl must match w_tbl");
    sptr = s_tbl->data_ptr<float>();
  }
  auto preds = torch::zeros({n_ex}, w_tbl.options());
  const int err = launch_vw_sgd_interact(
      idx.data_ptr<int>(), val.data_ptr<float>(), ns_off.data_ptr<long>(),
      col_seed.data_ptr<int>(), n_cols, pairs.data_ptr<int>(),
      pair_seed.data_ptr<int>(), n_pairs, (int)bits, label.data_ptr<float>(),
      wptr, w_tbl.data_ptr<float>(), g_tbl.data_ptr<float>(), sptr, (float)lr,
      (float)l2, (float)power_t, (int)loss, invariant ? 1 : 0, n_ex,
      preds.data_ptr<float>(), cur_stream());
  TORCH_CHECK(err == 0, "vw_sgd_interact launch failed: ",
              err < 0 ? "too many pairs" : hipGetErrorString((hipError_t)err));
  return preds;
}

torch::Tensor vw_predict_interact(
    torch::Tensor idx, torch::Tensor val, torch::Tensor ns_off,
    torch::Tensor col_seed, torch::Tensor pairs, torch::Tensor pair_seed,
    long bits, torch::Tensor w_tbl) {
  auto [n_ex, n_cols, n_pairs] = check_vw_interact(
      idx, val, ns_off, col_seed, pairs, pair_seed, bits, w_tbl);
  auto out = torch::zeros({n_ex}, w_tbl.options());
  const int err = launch_vw_predict_interact(
      idx.data_ptr<int>(), val.data_ptr<float>(), ns_off.data_ptr<long>(),
      col_seed.data_ptr<int>(), n_cols, pairs.data_ptr<int>(),
      pair_seed.data_ptr<int>(), n_pairs, (int)bits, w_tbl.data_ptr<float>(),
      n_ex, out.data_ptr<float>(), cur_stream());
  TORCH_CHECK(err == 0, "vw_predict_interact launch failed: ",
              err < 0 ? "too many pairs" : hipGetErrorString((hipError_t)err));
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
// wave-cooperative row chunks + in-kernel leaf totals
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

// ---------------------------------------------------------------------- ALS
// als_kernels.hip.  The CSR structure and the column range are checked by the
// caller (ops/backend.py); shapes, dtypes and scalars here.
static const int kAlsMaxK = 64;

static void als_check_factors(const torch::Tensor& Y, const char* name) {
  CHECK_DEV(Y); CHECK_CONTIG(Y);
  TORCH_CHECK(Y.dtype() == torch::kFloat32 && Y.dim() == 2 && Y.size(1) >= 1 &&
              Y.size(1) <= kAlsMaxK && Y.size(0) < (1L << 31), name,
              " must be (n, k) float32 with 1 <= k <= ", kAlsMaxK);
}

// G = Y^T Y, (k, k) float32, the same bits on every call.
torch::Tensor als_gram(torch::Tensor Y) {
  als_check_factors(Y, "Y");
  const long n = Y.size(0), k = Y.size(1);
  if (n == 0) return torch::zeros({k, k}, Y.options());
  const long K = k <= 32 ? 32 : 64;
  auto partial = torch::empty({als_gram_blocks(n) * K * K}, Y.options());
  auto G = torch::empty({k, k}, Y.options());
  const int err = launch_als_gram(Y.data_ptr<float>(), n, (int)k,
                                  partial.data_ptr<float>(),
                                  G.data_ptr<float>(), cur_stream());
  TORCH_CHECK(err == 0, "als_gram launch failed: ",
              hipGetErrorString((hipError_t)err));
  return G;
}

// x (rows, k): the solutions of one ALS half step.  heavy = 0 takes the
// kernels' ALS_HEAVY_DEGREE.
torch::Tensor als_half_step(torch::Tensor indptr, torch::Tensor col,
                            torch::Tensor val, torch::Tensor Y, double reg,
                            double alpha, bool implicit,
                            c10::optional<torch::Tensor> gram, long heavy) {
  sar_check_csr(indptr, col, &val, "als");
  als_check_factors(Y, "Y");
  const long n_rows = indptr.numel() - 1, k = Y.size(1);
  TORCH_CHECK(n_rows < (1L << 31), "too many rows");
  TORCH_CHECK(heavy >= 0, "heavy must be >= 0");
  const float* gp = nullptr;
  if (implicit) {
    TORCH_CHECK(gram.has_value(), "implicit mode needs gram = Y^T Y");
    const auto& g = *gram;
    CHECK_DEV(g); CHECK_CONTIG(g);
    TORCH_CHECK(g.dtype() == torch::kFloat32 && g.dim() == 2 &&
                g.size(0) == k && g.size(1) == k, "gram must be (k, k) float32");
    gp = g.data_ptr<float>();
  }
  auto x = torch::empty({n_rows, k}, Y.options());
  if (n_rows == 0) return x;
  const long thr = heavy == 0 ? als_heavy_degree() : heavy;
  int err = launch_als_solve_rows(
      indptr.data_ptr<long>(), col.data_ptr<int>(), val.data_ptr<float>(),
      Y.data_ptr<float>(), gp, (int)n_rows, (int)k, (float)reg, (float)alpha,
      implicit ? 1 : 0, thr, x.data_ptr<float>(), cur_stream());
  TORCH_CHECK(err == 0, "als_solve_rows launch failed: ",
              hipGetErrorString((hipError_t)err));
  auto degree = indptr.slice(0, 1) - indptr.slice(0, 0, n_rows);
  auto heavy_rows = torch::nonzero(degree > thr).flatten().to(torch::kInt32);
  if (heavy_rows.numel() > 0) {
    err = launch_als_solve_heavy(
        indptr.data_ptr<long>(), col.data_ptr<int>(), val.data_ptr<float>(),
        Y.data_ptr<float>(), gp, heavy_rows.data_ptr<int>(),
        (int)heavy_rows.numel(), (int)k, (float)reg, (float)alpha,
        implicit ? 1 : 0, x.data_ptr<float>(), cur_stream());
    TORCH_CHECK(err == 0, "als_solve_heavy launch failed: ",
                hipGetErrorString((hipError_t)err));
  }
  return x;
}

// Standardised anomaly score of (user, res) pairs over the tenants' factor
// tables laid end to end; NaN for tenant < 0 or an index outside its tables.
torch::Tensor als_score_pairs(torch::Tensor U, torch::Tensor V,
                              torch::Tensor user, torch::Tensor res,
                              torch::Tensor tenant, torch::Tensor u_off,
                              torch::Tensor v_off, torch::Tensor mean,
                              torch::Tensor sd) {
  for (const torch::Tensor* t : {&U, &V, &user, &res, &tenant, &u_off, &v_off,
                                 &mean, &sd}) {
    TORCH_CHECK(t->is_cuda() && t->is_contiguous(),
                "als_score_pairs arguments must be contiguous GPU tensors");
  }
  TORCH_CHECK(U.dtype() == torch::kFloat32 && V.dtype() == torch::kFloat32 &&
              U.dim() == 2 && V.dim() == 2 && U.size(1) == V.size(1) &&
              U.size(1) >= 1 && U.size(1) < (1L << 31),
              "U and V must be (n, k) float32 of one rank");
  const long n = user.numel(), T = mean.numel();
  TORCH_CHECK(user.dtype() == torch::kInt32 && res.dtype() == torch::kInt32 &&
              tenant.dtype() == torch::kInt32 && user.dim() == 1 &&
              res.dim() == 1 && tenant.dim() == 1 && res.numel() == n &&
              tenant.numel() == n, "user, res and tenant must be (n,) int32");
  TORCH_CHECK(u_off.dtype() == torch::kInt64 && v_off.dtype() == torch::kInt64 &&
              u_off.dim() == 1 && v_off.dim() == 1 && u_off.numel() == T + 1 &&
              v_off.numel() == T + 1 && T < (1L << 31),
              "u_off and v_off must be (tenants + 1,) int64");
  TORCH_CHECK(mean.dtype() == torch::kFloat64 && sd.dtype() == torch::kFloat64 &&
              mean.dim() == 1 && sd.dim() == 1 && sd.numel() == T,
              "mean and std must be (tenants,) float64");
  TORCH_CHECK(n < (1L << 39), "too many pairs for one launch");
  auto out = torch::empty({n}, U.options());
  if (n == 0) return out;
  const int err = launch_als_score_pairs(
      U.data_ptr<float>(), V.data_ptr<float>(), user.data_ptr<int>(),
      res.data_ptr<int>(), tenant.data_ptr<int>(), u_off.data_ptr<long>(),
      v_off.data_ptr<long>(), mean.data_ptr<double>(), sd.data_ptr<double>(),
      (int)T, (int)U.size(1), n, out.data_ptr<float>(), cur_stream());
  TORCH_CHECK(err == 0, "als_score_pairs launch failed: ",
              hipGetErrorString((hipError_t)err));
  return out;
}

// --------------------------------------------------------------- explainers
// explain_kernels.hip.  The contents of bidx and classes are range-checked by
// the caller (ops/backend.py); the kernel clamps bidx and node features again,
// and a class outside the outputs yields 0.
static const int kExplainMaxFeatures = 256;
static const int kExplainMaxOutputs = 8;
static const int kExplainMaxTileNodes = 6144;

static void explain_check(const torch::Tensor& t, const char* name,
                          torch::ScalarType dtype, int dim,
                          const torch::Tensor& X) {
  TORCH_CHECK(t.is_cuda() && t.device() == X.device(), "coalition_values: ",
              name, " must be on X's GPU");
  TORCH_CHECK(t.is_contiguous(), "coalition_values: ", name,
              " must be contiguous");
  TORCH_CHECK(t.scalar_type() == dtype, "coalition_values: ", name,
              " must be ", c10::toString(dtype));
  TORCH_CHECK(t.dim() == dim, "coalition_values: ", name, " must have ", dim,
              " dimension(s)");
}

torch::Tensor coalition_values(
    torch::Tensor feat, torch::Tensor thr, torch::Tensor left,
    torch::Tensor right, torch::Tensor val, torch::Tensor offsets,
    torch::Tensor tw, c10::optional<torch::Tensor> cat_offset,
    c10::optional<torch::Tensor> cat_words, long n_outputs, long t0, long t1,
    torch::Tensor X, torch::Tensor bg, torch::Tensor masks,
    c10::optional<torch::Tensor> bidx, long B, torch::Tensor base,
    long transform, double sigmoid, torch::Tensor classes, long tile_nodes) {
  explain_check(feat, "feature", torch::kInt32, 1, X);
  explain_check(thr, "threshold", torch::kFloat32, 1, X);
  explain_check(left, "left", torch::kInt32, 1, X);
  explain_check(right, "right", torch::kInt32, 1, X);
  explain_check(val, "value", torch::kFloat32, 1, X);
  explain_check(offsets, "offsets", torch::kInt64, 1, X);
  explain_check(tw, "weights", torch::kFloat32, 1, X);
  explain_check(X, "X", torch::kFloat32, 2, X);
  explain_check(bg, "bg", torch::kFloat32, 2, X);
  explain_check(masks, "masks", torch::kInt32, 3, X);
  explain_check(base, "base", torch::kFloat32, 1, X);
  explain_check(classes, "classes", torch::kInt32, 1, X);
  const long n_nodes = feat.numel();
  const long T = offsets.numel() - 1;
  TORCH_CHECK(thr.numel() == n_nodes && left.numel() == n_nodes &&
              right.numel() == n_nodes && val.numel() == n_nodes,
              "coalition_values: the node arrays must have one length");
  TORCH_CHECK(T >= 0 && tw.numel() == T,
              "coalition_values: weights must hold one weight per tree");
  TORCH_CHECK(0 <= t0 && t0 <= t1 && t1 <= T,
              "coalition_values: tree range must satisfy 0 <= t0 <= t1 <= T");
  TORCH_CHECK(n_outputs >= 1 && n_outputs <= kExplainMaxOutputs,
              "coalition_values: n_outputs must be in [1, ",
              kExplainMaxOutputs, "]");
  TORCH_CHECK(base.numel() == n_outputs,
              "coalition_values: base must hold one value per output");
  const long R = X.size(0), nf = X.size(1), nb = bg.size(0);
  TORCH_CHECK(nf >= 1 && nf <= kExplainMaxFeatures,
              "coalition_values: feature count must be in [1, ",
              kExplainMaxFeatures, "]");
  TORCH_CHECK(bg.size(1) == nf && nb >= 1 && nb < (1L << 31) / nf,
              "coalition_values: bg must be (nb >= 1, nf)");
  TORCH_CHECK(R <= 65535, "coalition_values: at most 65535 rows per call");
  const long Rm = masks.size(0), nZ = masks.size(1), W = masks.size(2);
  TORCH_CHECK(W == (nf + 31) / 32,
              "coalition_values: masks must have ceil(nf / 32) words");
  TORCH_CHECK(Rm == 1 || Rm == R,
              "coalition_values: masks must have 1 or R rows");
  TORCH_CHECK(B >= 1 && B < (1L << 24),
              "coalition_values: B must be at least 1");
  TORCH_CHECK(nZ < (1L << 31) / B,
              "coalition_values: too many coalitions x draws");
  const int* bi = nullptr;
  if (bidx.has_value()) {
    explain_check(*bidx, "bidx", torch::kInt32, 3, X);
    TORCH_CHECK(bidx->size(0) == R && bidx->size(1) == nZ &&
                bidx->size(2) == B,
                "coalition_values: bidx must be (R, nZ, B)");
    bi = bidx->data_ptr<int>();
  } else {
    TORCH_CHECK(B == nb, "coalition_values: without bidx the background is "
                "cycled, which needs B == nb");
  }
  TORCH_CHECK(transform >= 0 && transform <= 2,
              "coalition_values: transform must be 0, 1 or 2");
  TORCH_CHECK(transform != 1 || n_outputs == 1,
              "coalition_values: the binary sigmoid needs n_outputs == 1");
  TORCH_CHECK(transform != 2 || n_outputs >= 2,
              "coalition_values: softmax needs n_outputs >= 2");
  const long C = classes.numel();
  TORCH_CHECK(tile_nodes >= 0 && tile_nodes <= kExplainMaxTileNodes,
              "coalition_values: tile_nodes must be in [0, ",
              kExplainMaxTileNodes, "] (0 = automatic)");
  auto [co, cw] = cat_ptrs(cat_offset, cat_words);
  if (co != nullptr) {
    explain_check(*cat_offset, "cat_offset", torch::kInt32, 1, X);
    explain_check(*cat_words, "cat_words", torch::kInt32, 1, X);
    TORCH_CHECK(cat_offset->numel() == n_nodes,
                "coalition_values: cat_offset must hold one entry per node");
  }
  auto out = torch::empty({R, nZ, C}, X.options().dtype(torch::kFloat64));
  if (R == 0 || nZ == 0 || C == 0) return out;
  const int dsplit = explain_draw_splits(R, nZ, (int)B);
  auto part = torch::empty({dsplit > 1 ? R * nZ * dsplit * C : 0},
                           out.options());
  const int err = launch_coalition_values(
      feat.data_ptr<int>(), thr.data_ptr<float>(), left.data_ptr<int>(),
      right.data_ptr<int>(), val.data_ptr<float>(), offsets.data_ptr<long>(),
      tw.data_ptr<float>(), co, cw, n_nodes, (int)t0, (int)t1, (int)n_outputs,
      X.data_ptr<float>(), R, bg.data_ptr<float>(), (int)nb, (int)nf,
      (const unsigned*)masks.data_ptr<int>(), (int)Rm, (int)nZ, bi, (int)B,
      base.data_ptr<float>(), (int)transform, (float)sigmoid,
      classes.data_ptr<int>(), (int)C, (int)tile_nodes,
      part.data_ptr<double>(), out.data_ptr<double>(), cur_stream());
  TORCH_CHECK(err == 0, "coalition_values launch failed: ",
              err < 0 ? "argument out of range"
                      : hipGetErrorString((hipError_t)err));
  return out;
}

// ---------------------------------------------------------------- superpixels
// superpixel_kernels.hip.  Limits: at most kSlicMaxK centres per image; image
// sides at most kSlicMaxDim, which keeps a block's 32-bit LDS partial sums
// (at most 1024 pixels of at most max(255, side - 1) each) below 2^25; and
// H * W < 2^31.
static const int kSlicMaxK = 4096;
static const int kSlicMaxDim = 32768;

// Grid seeds along one axis: cell/2, cell/2 + cell, ... below n.
static long slic_grid(long n, long cell) {
  return n > cell / 2 ? (n - cell / 2 + cell - 1) / cell : 0;
}

static long slic_num_centers(long H, long W, long cell) {
  TORCH_CHECK(cell >= 1, "slic_segment: cell size must be positive");
  return slic_grid(H, cell) * slic_grid(W, cell);
}

// src: the column's pixels end to end, uint8 on the GPU.  shapes: CPU int64
// (n_img, 5) rows {byte offset into src, H, W, C, cell size}.  centres: optional
// (total K, 5) float32 start centres, image after image; seeded from the grid
// when absent.  Returns the labels of the last assignment, (total pixels,)
// int32, and the centres after the last update, (total K, 5) float32.
std::tuple<torch::Tensor, torch::Tensor> slic_segment(
    torch::Tensor src, torch::Tensor shapes,
    c10::optional<torch::Tensor> centres, double modifier, long n_iter) {
  CHECK_DEV(src); CHECK_CONTIG(src);
  TORCH_CHECK(src.dtype() == torch::kUInt8 && src.dim() == 1,
              "slic_segment: src must be a flat uint8 buffer");
  TORCH_CHECK(!shapes.is_cuda() && shapes.dtype() == torch::kInt64 &&
              shapes.dim() == 2 && shapes.size(1) == 5 &&
              shapes.is_contiguous(),
              "slic_segment: shapes must be a CPU int64 (n, 5) tensor");
  TORCH_CHECK(modifier > 0 && std::isfinite((float)modifier) &&
              (float)modifier > 0.f,
              "slic_segment: modifier must be positive and finite");
  TORCH_CHECK(n_iter >= 0 && n_iter <= 1000,
              "slic_segment: n_iter must lie in [0, 1000]");
  const long n = shapes.size(0);
  TORCH_CHECK(n < (1L << 20), "slic_segment: too many images for one launch");
  auto desc = torch::empty({n * 8 + n + 1}, shapes.options());
  long* d = desc.data_ptr<long>();
  long* wo = d + n * 8;
  const long* s = shapes.data_ptr<long>();
  long total_k = 0, total_pix = 0, items = 0, max_k = 0;
  for (long i = 0; i < n; ++i) {
    const long off = s[5 * i], H = s[5 * i + 1], W = s[5 * i + 2],
               C = s[5 * i + 3], cell = s[5 * i + 4];
    TORCH_CHECK(cell >= 1 && cell <= kSlicMaxDim,
                "slic_segment: cell size out of range");
    TORCH_CHECK(H >= 1 && W >= 1 && H <= kSlicMaxDim && W <= kSlicMaxDim &&
                H * W < (1L << 31),
                "slic_segment: image sides must lie in [1, ", kSlicMaxDim,
                "] (the 32-bit LDS partial sums) with H * W < 2^31");
    TORCH_CHECK(C == 1 || C == 3, "slic_segment: images have 1 or 3 channels");
    TORCH_CHECK(off >= 0 && off + H * W * C <= src.numel(),
                "slic_segment: image runs past the source buffer");
    const long K = slic_num_centers(H, W, cell);
    TORCH_CHECK(K >= 1 && K <= kSlicMaxK, "slic_segment: an image must have "
                "between 1 and ", kSlicMaxK, " centres, got ", K);
    long* q = d + 8 * i;
    q[0] = off; q[1] = H; q[2] = W; q[3] = C; q[4] = K; q[5] = total_k;
    q[6] = total_pix; q[7] = cell;
    wo[i] = items;
    total_k += K;
    total_pix += H * W;
    items += (H * W + 1023) / 1024;
    max_k = std::max(max_k, K);
  }
  wo[n] = items;
  TORCH_CHECK(items < (1L << 31), "slic_segment: column too large for one "
              "launch");
  // without an iteration nothing is assigned: every label is 0
  auto lopt = src.options().dtype(torch::kInt32);
  auto labels = n_iter == 0 ? torch::zeros({total_pix}, lopt)
                            : torch::empty({total_pix}, lopt);
  torch::Tensor ctr;
  if (centres.has_value()) {
    TORCH_CHECK(centres->is_cuda() && centres->device() == src.device() &&
                centres->dtype() == torch::kFloat32 && centres->dim() == 2 &&
                centres->size(0) == total_k && centres->size(1) == 5,
                "slic_segment: centres must be (total K, 5) float32 beside "
                "src");
    ctr = centres->contiguous().clone();
  } else {
    ctr = torch::empty({total_k, 5}, src.options().dtype(torch::kFloat32));
  }
  if (n == 0) return {labels, ctr};
  auto sums = torch::zeros({total_k, 6}, src.options().dtype(torch::kInt64));
  auto ddesc = desc.to(src.device());
  const long* dd = ddesc.data_ptr<long>();
  const int err = launch_slic_segment(
      src.data_ptr<uint8_t>(), src.numel(), dd, dd + n * 8, (int)n, items,
      (int)max_k, total_k, ctr.data_ptr<float>(),
      (unsigned long long*)sums.data_ptr<int64_t>(), labels.data_ptr<int>(),
      total_pix, (float)modifier, (int)n_iter,
      centres.has_value() ? 0 : 1, cur_stream());
  TORCH_CHECK(err == 0, "slic_segment launch failed: ",
              err < 0 ? "argument out of range"
                      : hipGetErrorString((hipError_t)err));
  return {labels, ctr};
}

// (n, 3, size, size) float32: sample s is the image with every segment whose
// bit in states[s] is clear replaced by `fill`, gray replicated, mapped
// through lut, CHW, and resized bilinearly when the image is not size x size.
torch::Tensor masked_image_batch(torch::Tensor img, torch::Tensor seg,
                                 torch::Tensor states, long m, long fill,
                                 long size, torch::Tensor lut) {
  for (const torch::Tensor* t : {&img, &seg, &states, &lut}) {
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                t->device() == img.device(), "masked_image_batch arguments "
                "must be contiguous tensors on one GPU");
  }
  TORCH_CHECK(img.dtype() == torch::kUInt8 &&
              (img.dim() == 2 || (img.dim() == 3 && (img.size(2) == 1 ||
                                                     img.size(2) == 3))),
              "masked_image_batch: image must be uint8 (H, W) or (H, W, 1|3)");
  const long H = img.size(0), W = img.size(1);
  const long C = img.dim() == 3 ? img.size(2) : 1;
  TORCH_CHECK(H >= 1 && W >= 1 && H <= kSlicMaxDim && W <= kSlicMaxDim &&
              H * W < (1L << 31), "masked_image_batch: image too large");
  TORCH_CHECK(seg.dtype() == torch::kInt32 && seg.dim() == 2 &&
              seg.size(0) == H && seg.size(1) == W,
              "masked_image_batch: segments must be int32 (H, W)");
  TORCH_CHECK(m >= 1 && m <= kSlicMaxK,
              "masked_image_batch: segment count must lie in [1, ", kSlicMaxK,
              "]");
  TORCH_CHECK(states.dtype() == torch::kInt32 && states.dim() == 2 &&
              states.size(1) == (m + 31) / 32 && states.size(0) < (1L << 31),
              "masked_image_batch: states must be int32 (n, ceil(m / 32))");
  TORCH_CHECK(fill >= 0 && fill <= 255,
              "masked_image_batch: fill must lie in [0, 255]");
  TORCH_CHECK(size >= 1 && size <= kSlicMaxDim && size * size < (1L << 31),
              "masked_image_batch: size out of range");
  TORCH_CHECK(lut.dtype() == torch::kFloat32 && lut.numel() == 256,
              "masked_image_batch: lut must hold 256 float32 values");
  const long n = states.size(0);
  auto out = torch::empty({n, 3, size, size},
                          img.options().dtype(torch::kFloat32));
  if (n == 0) return out;
  const int err = launch_masked_image_batch(
      img.data_ptr<uint8_t>(), (int)H, (int)W, (int)C, seg.data_ptr<int>(),
      (const unsigned*)states.data_ptr<int>(), (int)n, (int)states.size(1),
      (int)m, (int)fill, (int)size, lut.data_ptr<float>(),
      out.data_ptr<float>(), cur_stream());
  TORCH_CHECK(err == 0, "masked_image_batch launch failed: ",
              err < 0 ? "argument out of range"
                      : hipGetErrorString((hipError_t)err));
  return out;
}

// ---------------------------------------------------------- isolation forest
// iforest_kernels.hip: one block grows one tree into a padded slab, a cumsum
// over the node counts and one gather kernel make the compact forest.  The
// only host wait is the read of the total node count that sizes the result.
std::vector<torch::Tensor> iforest_build(torch::Tensor X, long n_trees,
                                         long sub_n, long n_feat,
                                         bool bootstrap, int64_t seed) {
  CHECK_DEV(X); CHECK_CONTIG(X);
  TORCH_CHECK(X.dtype() == torch::kFloat32 && X.dim() == 2,
              "X must be (n, nf) float32");
  const long n = X.size(0), nf = X.size(1);
  TORCH_CHECK(n < (1L << 31) && nf >= 1 && nf < (1L << 24), "X too large");
  TORCH_CHECK(sub_n >= 2 && sub_n <= iforest_max_sub() && sub_n <= n,
              "sub_n out of range");
  TORCH_CHECK(n_feat >= 1 && n_feat <= nf, "n_feat out of range");
  TORCH_CHECK(n_trees >= 1 && n_trees < (1L << 20), "n_trees out of range");
  const long cap = 2 * sub_n - 1;
  const auto i32 = X.options().dtype(torch::kInt32);
  auto rows = torch::empty({n_trees, sub_n}, i32);
  auto slab_i = torch::empty({5, n_trees, cap}, i32);
  auto slab_t = torch::empty({n_trees, cap}, X.options());
  auto count = torch::empty({n_trees}, i32);
  int* si = slab_i.data_ptr<int>();
  const long plane = n_trees * cap;
  int err = launch_iforest_build(
      X.data_ptr<float>(), n, (int)nf, (int)n_trees, (int)sub_n, (int)n_feat,
      bootstrap ? 1 : 0, (unsigned long long)seed, rows.data_ptr<int>(), si,
      slab_t.data_ptr<float>(), si + plane, si + 2 * plane, si + 3 * plane,
      si + 4 * plane, count.data_ptr<int>(), cur_stream());
  TORCH_CHECK(err == 0, "iforest_build launch failed: ",
              hipGetErrorString((hipError_t)err));
  auto offsets = torch::zeros({n_trees + 1}, X.options().dtype(torch::kInt64));
  offsets.slice(0, 1).copy_(count.cumsum(0, torch::kInt64));
  const long total = offsets[n_trees].item<int64_t>();
  TORCH_CHECK(total >= n_trees && total <= plane, "iforest_build: bad counts");
  auto out_i = torch::empty({5, total}, i32);
  auto out_t = torch::empty({total}, X.options());
  int* oi = out_i.data_ptr<int>();
  err = launch_iforest_compact(
      si, slab_t.data_ptr<float>(), si + plane, si + 2 * plane,
      si + 3 * plane, si + 4 * plane, offsets.data_ptr<int64_t>(),
      (int)n_trees, (int)cap, oi, out_t.data_ptr<float>(), oi + total,
      oi + 2 * total, oi + 3 * total, oi + 4 * total, cur_stream());
  TORCH_CHECK(err == 0, "iforest_compact launch failed: ",
              hipGetErrorString((hipError_t)err));
  return {rows, out_i[0], out_t, out_i[1], out_i[2], out_i[3], out_i[4],
          offsets};
}

// ------------------------------------------------------------------ LIME fit
// lime_fit_kernels.hip: every kernel-weighted lasso surrogate of a chunk in
// one launch, one block per explained row.  states (R, n, ceil(m / 32)) int32
// bit rows, scores (R, n, C) float64.  Returns coef (R, C, m), intercept,
// r2 (R, C) float64 and n_sweeps (R, C) int32.
std::vector<torch::Tensor> lime_fit(torch::Tensor states, long m,
                                    torch::Tensor scores, double kernel_width,
                                    double alpha, long max_iter, double tol) {
  CHECK_DEV(states); CHECK_CONTIG(states);
  CHECK_DEV(scores); CHECK_CONTIG(scores);
  TORCH_CHECK(states.device() == scores.device(),
              "lime_fit: states and scores must share a GPU");
  TORCH_CHECK(m >= 1 && m <= lime_fit_max_features(),
              "lime_fit: m must lie in [1, ", lime_fit_max_features(), "]");
  TORCH_CHECK(states.dtype() == torch::kInt32 && states.dim() == 3 &&
              states.size(2) == (m + 31) / 32,
              "lime_fit: states must be int32 (R, n, ceil(m / 32))");
  const long R = states.size(0), n = states.size(1);
  TORCH_CHECK(scores.dtype() == torch::kFloat64 && scores.dim() == 3 &&
              scores.size(0) == R && scores.size(1) == n,
              "lime_fit: scores must be float64 (R, n, C)");
  const long C = scores.size(2);
  TORCH_CHECK(C >= 1 && C <= lime_fit_max_outputs(),
              "lime_fit: C must lie in [1, ", lime_fit_max_outputs(), "]");
  TORCH_CHECK(n >= 1 && n < (1L << 31) && R < (1L << 31),
              "lime_fit: n must lie in [1, 2^31) and R below 2^31");
  TORCH_CHECK(kernel_width > 0 && alpha >= 0 && tol == tol &&
              max_iter >= 0 && max_iter < (1L << 31),
              "lime_fit: kernel_width > 0, alpha >= 0, max_iter >= 0");
  const auto f64 = scores.options();
  auto coef = torch::empty({R, C, m}, f64);
  auto intercept = torch::empty({R, C}, f64);
  auto r2 = torch::empty({R, C}, f64);
  auto sweeps = torch::empty({R, C}, f64.dtype(torch::kInt32));
  if (R == 0) return {coef, intercept, r2, sweeps};
  const long per_row = lime_fit_scratch_doubles((int)m);
  auto scratch = torch::empty({R * per_row}, f64);
  const int err = launch_lime_fit(
      states.data_ptr<int>(), scores.data_ptr<double>(), (int)R, (int)n,
      (int)m, (int)C, kernel_width, alpha, (int)max_iter, tol,
      per_row ? scratch.data_ptr<double>() : nullptr, coef.data_ptr<double>(),
      intercept.data_ptr<double>(), r2.data_ptr<double>(),
      sweeps.data_ptr<int>(), cur_stream());
  TORCH_CHECK(err == 0, "lime_fit launch failed: ",
              err < 0 ? "argument out of range"
                      : hipGetErrorString((hipError_t)err));
  return {coef, intercept, r2, sweeps};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("hist_build", &hist_build, "per-leaf (feature,bin) grad/hess/count histogram");
  m.def("hist_build_fixed_pair", &hist_build_fixed_pair,
        "fixed-point histogram over paired (8-feature) planes");
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
  m.def("vw_sgd_minibatch_interact", &vw_sgd_minibatch_interact,
        "adaptive sparse SGD minibatch, namespace pairs crossed in-kernel");
  m.def("vw_predict_interact", &vw_predict_interact,
        "sparse linear predict, namespace pairs crossed in-kernel");
  m.def("vw_interact_window", &vw_interact_window,
        "entries of one example held in LDS by the interact kernels");
  m.def("vw_interact_max_pairs", &vw_interact_max_pairs,
        "most namespace pairs one interact launch takes");
  m.def("tree_shap", &tree_shap, "path-dependent TreeSHAP contributions");
  m.def("tree_shap_csr", &tree_shap_csr,
        "TreeSHAP over CSR rows, compact per-used-feature contributions");
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
  m.def("coalition_values", &coalition_values,
        "mean transformed forest output per (row, coalition), samples never "
        "built");
  m.attr("EXPLAIN_MAX_FEATURES") = kExplainMaxFeatures;
  m.attr("EXPLAIN_MAX_OUTPUTS") = kExplainMaxOutputs;
  m.attr("EXPLAIN_MAX_TILE_NODES") = kExplainMaxTileNodes;
  m.def("als_gram", &als_gram, "Y^T Y in fixed summation order");
  m.def("als_half_step", &als_half_step,
        "one ALS half step: per-row normal equations formed and solved fused",
        py::arg("indptr"), py::arg("col"), py::arg("val"), py::arg("Y"),
        py::arg("reg"), py::arg("alpha"), py::arg("implicit"),
        py::arg("gram") = py::none(), py::arg("heavy") = 0);
  m.def("als_score_pairs", &als_score_pairs,
        "standardised -U.V of (user, resource) pairs over tenant tables");
  m.def("als_heavy_degree", &als_heavy_degree,
        "row degree above which a whole block takes a row");
  m.def("slic_segment", &slic_segment,
        "SLIC superpixels of a column of uint8 images, exact integer means",
        py::arg("src"), py::arg("shapes"), py::arg("centres") = py::none(),
        py::arg("modifier") = 10.0, py::arg("n_iter") = 5);
  m.def("slic_num_centers", &slic_num_centers,
        "grid-seeded centres of an H x W image at a cell size");
  m.def("masked_image_batch", &masked_image_batch,
        "masked samples of one image as the model's float32 NCHW batch");
  m.def("iforest_build", &iforest_build,
        "grow an isolation forest, one block per tree, compact level-order "
        "arrays");
  m.def("iforest_staged", &iforest_staged,
        "1 when a tree's sample of sub_n x nf values is staged in LDS");
  m.attr("IFOREST_MAX_SUB") = iforest_max_sub();
  m.def("lime_fit", &lime_fit,
        "kernel-weighted lasso surrogates of a chunk of LIME rows, one launch");
  m.attr("LIME_FIT_MAX_FEATURES") = lime_fit_max_features();
  m.attr("LIME_FIT_MAX_OUTPUTS") = lime_fit_max_outputs();
  m.attr("SLIC_MAX_K") = kSlicMaxK;
  m.attr("SLIC_MAX_DIM") = kSlicMaxDim;
  m.attr("ALS_MAX_K") = kAlsMaxK;
  m.attr("SAR_MAX_K") = kSarMaxK;
  m.attr("SAR_MAX_TILE") = kSarMaxTile;
}
