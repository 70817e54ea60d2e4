// Native leaf-wise tree-growth driver — the C++ runtime piece of the GBDT.
//
// Runs the entire leaf-wise loop in C++ with ONE Python call per tree,
// organized around two ideas:
//
//  * ARENA MODE: the tree's working set (paired bin planes + pre-quantized
//    (gq,hq) records + original row ids) lives in a per-tree DOUBLE-BUFFERED
//    arena.  Every split scatters the parent's segment into the other buffer
//    (stable left|right), so child histograms read CONTIGUOUS rows — the
//    sparse row gather that bounded child hist builds (measured 2.3x,
//    tools/hist_gather_probe.py) is gone; the cost is streaming ~124 B/row
//    of arena payload per split, which HBM3E absorbs.  Live leaves always
//    own disjoint row ranges, so two in-flight splits never overlap even
//    across buffers.  When the root row set is every row in order (no
//    bagging, no GOSS), the root reads its planes straight from the static
//    binned_pair — a third, read-only source — and only the gradient records
//    and row ids of buffer 0 are written per tree.
//
//  * SPECULATION: a popped leaf's split work is independent of processing
//    order (its split was fixed at creation), so the driver pre-launches the
//    next-best candidate's whole chain (count → scatter → smaller-child hist
//    → sibling subtract+scan → pinned readback behind a HIP event) while
//    the host waits on the current readback.  Commit order stays exactly
//    leaf-wise.  The chain never blocks the host: child ranges resolve from
//    the DEVICE-side left count, which rides back with the scan result.
//    Candidate order is deterministic across ranks, so the histogram
//    all_reduce order matches and speculation is safe in multi-rank mode.
//
//  * STREAM POOL: on a single rank the (up to three) chains in flight go
//    round-robin over the caller's stream and up to two pooled side streams
//    (MMLSPARK_AMD_GROWER_STREAMS, 1-3), so one leaf's LDS-atomic-bound
//    histogram can run next to another leaf's HBM-bound scatter.  Chains of
//    different leaves touch disjoint arena ranges and each has its own
//    counters, so they need no ordering among themselves.
//
// Categorical features fall back to the Python grower (models/gbdt/
// trainer.py).  Replaces the growth loop the reference delegates to
// LightGBM's serial_tree_learner behind LGBM_BoosterUpdateOneIter
// (SURVEY §2.1).
#include <torch/extension.h>
#include <torch/csrc/distributed/c10d/ProcessGroup.hpp>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <numeric>
#include <queue>
#include <vector>

extern "C" {
void launch_arena_gather(const void*, long, const float*, const float*,
                         const int*, long, int, double, double, void*, void*,
                         int*, hipStream_t);
void launch_partition_arena(const void*, const void*, const int*, void*,
                            void*, int*, long, int, long, long, int, int,
                            const unsigned*, int*, int*, long, int,
                            hipStream_t);
void launch_hist_pair_range(const void*, const void*, long, long, long,
                            long long*, int, int, int, const int*, int, long,
                            int, int, int, hipStream_t);
void launch_sibling_scan(const long long*, const long long*, long long*, int,
                         long, int, float, float, float, float, long,
                         const bool*, float*, double, double, hipStream_t);
void launch_apply_leaf_values(float*, long, const int*, const long*, int,
                              const float*, long, hipStream_t);
}

static hipStream_t grower_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

namespace {

constexpr int kMaxGrowerStreams = 3;
// default of MMLSPARK_AMD_GROWER_STREAMS (docs/benchmarks.md, stream sweep)
constexpr int kDefaultGrowerStreams = 3;

// Streams a tree's chains rotate over: [0] is the caller's stream, the rest
// come from torch's stream pool ONCE per process and device, so every tree
// reuses the same two side streams and, with the caller's, the grower never
// holds more than three (the runtime's default is four hardware queues).
std::vector<c10::hip::HIPStream> grower_streams(int n) {
  auto cur = c10::hip::getCurrentHIPStream();
  std::vector<c10::hip::HIPStream> out{cur};
  if (n <= 1) return out;
  static std::mutex mu;
  static std::vector<std::vector<c10::hip::HIPStream>> side;  // per device
  std::lock_guard<std::mutex> lock(mu);
  const size_t dev = (size_t)cur.device_index();
  if (side.size() <= dev) side.resize(dev + 1);
  while ((int)side[dev].size() < kMaxGrowerStreams - 1)
    side[dev].push_back(
        c10::hip::getStreamFromPool(false, cur.device_index()));
  for (int i = 0; i + 1 < n; ++i) out.push_back(side[dev][i]);
  return out;
}

int grower_streams_from_env() {
  const char* e = std::getenv("MMLSPARK_AMD_GROWER_STREAMS");
  if (!e || !*e) return kDefaultGrowerStreams;
  char* end = nullptr;
  const long v = std::strtol(e, &end, 10);
  TORCH_CHECK(*end == '\0' && v >= 1 && v <= kMaxGrowerStreams,
              "MMLSPARK_AMD_GROWER_STREAMS must be 1..", kMaxGrowerStreams,
              ", got '", e, "'");
  return (int)v;
}

// On/off switches of the tree's head and tail (docs/kernels.md); all default
// to on.  Read once per tree, before any launch.
bool grower_switch(const char* name) {
  const char* e = std::getenv(name);
  if (!e || !*e) return true;
  TORCH_CHECK((e[0] == '0' || e[0] == '1') && e[1] == '\0', name,
              " must be 0 or 1, got '", e, "'");
  return e[0] == '1';
}

// Block width, block order and LDS layout of the range histogram.  An
// explicit argument wins; else MMLSPARK_AMD_HIST_THREADS (0/256/512/1024),
// MMLSPARK_AMD_HIST_ORDER (0/1) and MMLSPARK_AMD_HIST_LAYOUT (0/1/2); else
// the launcher's policy (threads 0, order -1, layout -1).  The environment
// is read at every launch, so one process can switch settings: a getenv is
// nothing next to a kernel launch.
long hist_env(const char* name, long unset) {
  const char* e = std::getenv(name);
  if (!e || !*e) return unset;
  char* end = nullptr;
  const long v = std::strtol(e, &end, 10);
  TORCH_CHECK(*end == '\0' && v >= 0, name,
              " must be a non-negative integer, got '", e, "'");
  return v;
}

int hist_threads(long arg = 0) {
  const long v = arg != 0 ? arg : hist_env("MMLSPARK_AMD_HIST_THREADS", 0);
  TORCH_CHECK(v == 0 || v == 256 || v == 512 || v == 1024,
              "threads / MMLSPARK_AMD_HIST_THREADS must be 0, 256, 512 or "
              "1024, got ", v);
  return (int)v;
}

int hist_order(long arg = -1) {
  const long v = arg != -1 ? arg : hist_env("MMLSPARK_AMD_HIST_ORDER", -1);
  TORCH_CHECK(v >= -1 && v <= 1,
              "order / MMLSPARK_AMD_HIST_ORDER must be 0 or 1, got ", v);
  return (int)v;
}

int hist_layout(long arg = -1) {
  const long v = arg != -1 ? arg : hist_env("MMLSPARK_AMD_HIST_LAYOUT", -1);
  TORCH_CHECK(v >= -1 && v <= 2,
              "layout / MMLSPARK_AMD_HIST_LAYOUT must be 0, 1 or 2, got ", v);
  return (int)v;
}

struct GrowCtx {
  long n_arena;    // rows in the arena (= rows_root size after bagging)
  int n_bins;
  int npairs;
  int tail_bytes;  // valid feature-bytes in the last pair (zero-pad skipped)
  // double-buffered arena: [0]/[1]
  torch::Tensor pair[2];   // (npairs, n_arena) i64 paired bin planes
  // kRootBuf's planes: the static binned_pair when the root reads it in
  // place (never a scatter destination), else null
  const void* root_pair = nullptr;
  torch::Tensor ghq[2];    // (n_arena, 2) i64 (gq, CNT|hq)
  torch::Tensor rowid[2];  // (n_arena,) i32 original row ids
  long nf;
  double scale_g, scale_h;
  double l1, l2, min_data, min_hess, min_gain;
  int num_leaves, max_depth;
  torch::Tensor feat_mask;  // bool (nf_pad,) or undefined
  // c10d process group for the per-split histogram all_reduce — called from
  // C++ with NO GIL (the round-1 Python-callback hop is gone).  With the
  // NCCL(=RCCL) backend Work::wait() only blocks the current HIP stream, so
  // speculated histogram kernels keep overlapping the collective.
  c10::intrusive_ptr<c10d::ProcessGroup> pg;
  bool has_reduce;
  bool distributed;
  // categorical features (already filtered by the iteration's feature mask);
  // the host-side sorted one-vs-rest scan replicates trainer._cat_scan
  // bit-for-bit (float32 arithmetic, lexsort tie-break by bin id)
  std::vector<int> cat_feats;
  double cat_smooth = 10.0;
  torch::Tensor cat_idx_dev;  // i64 device indices for index_select
  // chains rotate over these streams; [0] is the caller's.  The partition
  // block counters and left count are reused in stream order, so every
  // stream has its own pair.
  std::vector<c10::hip::HIPStream> streams;
  size_t next_stream = 0;
  torch::Tensor scratch[kMaxGrowerStreams];
  torch::Tensor total[kMaxGrowerStreams];
  // per-tree histogram slabs, one slot per split: small children accumulate
  // into pre-zeroed slots, big children are written whole by the sibling scan
  torch::Tensor slab_zero, slab_raw;
  long slab_used_zero = 0, slab_used_raw = 0;
};

// LeafCand::buf of a root that reads the static planes.  Its gradient records
// and row ids are buffer 0's and its children go to buffer 1, so buffer 0's
// planes are first written by the root's grandchildren.
constexpr int kRootBuf = 2;

const void* pair_of(const GrowCtx& ctx, int buf) {
  return buf == kRootBuf ? ctx.root_pair : ctx.pair[buf].data_ptr();
}
int small_buf(int buf) { return buf == kRootBuf ? 0 : buf; }  // ghq, rowid
int child_buf(int buf) { return buf == kRootBuf ? 1 : buf ^ 1; }

struct SplitJob {
  torch::Tensor hist_l, hist_r;
  torch::Tensor scan_host;  // (nh, nf_pad, 6) f32 pinned per-feature records
  torch::Tensor nl_host;    // (1,) i32 pinned — local left count readback
  torch::Tensor cat_host;   // (nh, ncat, nb, 3) i64 pinned — cat hist rows
  torch::Tensor bits_host;  // (8,) i32 pinned — partition bitset staging
  torch::Tensor bits_dev;   // (8,) i32 device
  torch::Tensor row0_host;  // (nb, 3) i64 pinned — root: feature 0's hist row
  long nl_known = -1;       // host-known left count (single-rank fast path)
  hipEvent_t ev = nullptr;

  // A job that was speculated but never committed may still be in flight:
  // its pinned buffers are targets of raw hipMemcpyAsync calls the host
  // allocator knows nothing about, so they must outlive the chain.  For a
  // consumed job the event is long complete and this returns at once.
  ~SplitJob() {
    if (ev) {
      (void)hipEventSynchronize(ev);
      (void)hipEventDestroy(ev);
    }
  }
};

struct LeafCand {
  double gain = 0;
  long seq = 0;
  int node_id = 0;
  int depth = 0;
  long lo = 0, hi = 0;  // arena row range
  int buf = 0;          // which arena buffer holds this leaf's rows (0, 1
                        // or kRootBuf)
  torch::Tensor hist;   // int64 (nf_pad, nb, 3), globally reduced
  double G = 0, H = 0, C = 0;
  double GL = 0, HL = 0, CL = 0;
  int feat = -1, bin = 0;
  std::vector<int> cats;  // chosen category bins (empty = numeric split)
  std::shared_ptr<SplitJob> job;
};

using CandPtr = std::shared_ptr<LeafCand>;

struct CandCmp {
  bool operator()(const CandPtr& a, const CandPtr& b) const {
    if (a->gain != b->gain) return a->gain < b->gain;  // max-heap by gain
    return a->seq > b->seq;
  }
};

// a histogram slot from the per-tree slab; per-split allocation once
// speculation has used the slab up
torch::Tensor hist_slot(GrowCtx& ctx, bool zeroed) {
  torch::Tensor& slab = zeroed ? ctx.slab_zero : ctx.slab_raw;
  long& used = zeroed ? ctx.slab_used_zero : ctx.slab_used_raw;
  if (used < slab.size(0)) return slab.select(0, used++);
  auto opt = ctx.pair[0].options();
  return zeroed ? torch::zeros({ctx.npairs * 8, ctx.n_bins, 3}, opt)
                : torch::empty({ctx.npairs * 8, ctx.n_bins, 3}, opt);
}

// histogram over an arena segment [lo+?, ...) of buffer `buf`; side >= 0
// resolves the child sub-range from the device left count (no host sync)
torch::Tensor build_hist(GrowCtx& ctx, int buf, long lo, long m,
                         const int* nl_dev = nullptr, int side = -1) {
  auto hist = hist_slot(ctx, true);
  launch_hist_pair_range(
      pair_of(ctx, buf), ctx.ghq[small_buf(buf)].data_ptr(), ctx.n_arena, lo, m,
      (long long*)hist.data_ptr<int64_t>(), ctx.n_bins, ctx.npairs,
      ctx.tail_bytes, nl_dev, side, 0, hist_threads(), hist_order(),
      hist_layout(), grower_stream());
  if (ctx.has_reduce) {
    std::vector<at::Tensor> v{hist};
    ctx.pg->allreduce(v)->wait();  // stream-ordered on RCCL; no GIL
  }
  return hist;
}

// launch the fused sibling subtract + scan (parent undefined: scan `small`
// alone, the root); the per-feature records land in a pinned host buffer
// behind an event — no stream sync, the arg-max over features is the host's.
// row0: feature 0's row of `small` rides back too (the root's totals).
void launch_scan_async(GrowCtx& ctx, const torch::Tensor& parent,
                       const torch::Tensor& small, torch::Tensor big,
                       bool small_is_left, SplitJob& job, bool row0 = false) {
  const long nh = parent.defined() ? 2 : 1;
  const long nf_pad = small.size(0);
  auto records = torch::empty(
      {nh, nf_pad, 6},
      torch::TensorOptions().dtype(torch::kFloat32).device(small.device()));
  const bool* mask = ctx.feat_mask.defined()
                         ? ctx.feat_mask.data_ptr<bool>() : nullptr;
  launch_sibling_scan(
      parent.defined() ? (const long long*)parent.data_ptr<int64_t>()
                       : nullptr,
      (const long long*)small.data_ptr<int64_t>(),
      big.defined() ? (long long*)big.data_ptr<int64_t>() : nullptr,
      small_is_left ? 1 : 0, nf_pad, ctx.n_bins, (float)ctx.l1, (float)ctx.l2,
      (float)ctx.min_data, (float)ctx.min_hess, ctx.nf, mask,
      records.data_ptr<float>(), 1.0 / ctx.scale_g, 1.0 / ctx.scale_h,
      grower_stream());
  job.scan_host = torch::empty({nh, nf_pad, 6}, torch::TensorOptions()
                                                    .dtype(torch::kFloat32)
                                                    .pinned_memory(true));
  (void)hipMemcpyAsync(job.scan_host.data_ptr<float>(),
                       records.data_ptr<float>(),
                       nh * nf_pad * 6 * sizeof(float), hipMemcpyDeviceToHost,
                       grower_stream());
  if (!ctx.cat_feats.empty()) {
    // categorical rows of the reduced histogram ride back with the scan;
    // the sorted one-vs-rest scan runs on host at commit (≤ ncat×256 bins)
    const long ncat = (long)ctx.cat_feats.size();
    const size_t per_hist = (size_t)ncat * ctx.n_bins * 3;
    job.cat_host = torch::empty({nh, ncat, (long)ctx.n_bins, 3},
                                torch::TensorOptions()
                                    .dtype(torch::kInt64)
                                    .pinned_memory(true));
    for (long h = 0; h < nh; ++h) {
      const torch::Tensor& src = (h == 0) == small_is_left ? small : big;
      auto cat_rows = src.index_select(0, ctx.cat_idx_dev).contiguous();
      (void)hipMemcpyAsync(job.cat_host.data_ptr<int64_t>() + h * per_hist,
                           cat_rows.data_ptr<int64_t>(),
                           per_hist * sizeof(int64_t), hipMemcpyDeviceToHost,
                           grower_stream());
    }
  }
  if (row0) {
    job.row0_host = torch::empty({(long)ctx.n_bins, 3}, torch::TensorOptions()
                                                            .dtype(torch::kInt64)
                                                            .pinned_memory(true));
    (void)hipMemcpyAsync(job.row0_host.data_ptr<int64_t>(),
                         small.data_ptr<int64_t>(),
                         (size_t)ctx.n_bins * 3 * sizeof(int64_t),
                         hipMemcpyDeviceToHost, grower_stream());
  }
  (void)hipEventCreateWithFlags(&job.ev, hipEventDisableTiming);
  (void)hipEventRecord(job.ev, grower_stream());
}

struct CatBest {
  float gain = -INFINITY;
  int feat = -1;
  float GL = 0, HL = 0, CL = 0;
  std::vector<int> cats;
};

// Bit-for-bit replica of trainer._cat_scan: float32 arithmetic, sequential
// float32 cumsums, lexsort tie-break by bin id, first-max argmax.
CatBest cat_scan_host(const GrowCtx& ctx, const int64_t* hist) {
  CatBest best;
  const int nb = ctx.n_bins;
  const double inv_g = 1.0 / ctx.scale_g, inv_h = 1.0 / ctx.scale_h;
  for (size_t ci = 0; ci < ctx.cat_feats.size(); ++ci) {
    const int64_t* h = hist + ci * (size_t)nb * 3;
    std::vector<int> present;
    for (int b = 0; b < nb; ++b)
      if (h[b * 3 + 2] > 0) present.push_back(b);
    const int m = (int)present.size();
    if (m < 2) continue;
    std::vector<float> g(m), hh(m), c(m), ratio(m);
    for (int i = 0; i < m; ++i) {
      const int b = present[i];
      g[i] = (float)((double)h[b * 3 + 0] * inv_g);
      hh[i] = (float)((double)h[b * 3 + 1] * inv_h);
      c[i] = (float)h[b * 3 + 2];
      ratio[i] = g[i] / (hh[i] + (float)ctx.cat_smooth);
    }
    std::vector<int> order(m);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
      if (ratio[x] != ratio[y]) return ratio[x] < ratio[y];
      return present[x] < present[y];
    });
    std::vector<float> GL(m), HL(m), CL(m);
    float ag = 0.f, ah = 0.f, ac = 0.f;
    for (int i = 0; i < m; ++i) {
      ag += g[order[i]]; ah += hh[order[i]]; ac += c[order[i]];
      GL[i] = ag; HL[i] = ah; CL[i] = ac;
    }
    const float G = GL[m - 1], H = HL[m - 1], C = CL[m - 1];
    auto sc = [&](float Gs, float Hs) {
      const float Ga = std::max(std::fabs(Gs) - (float)ctx.l1, 0.0f);
      return Ga * Ga / (Hs + (float)ctx.l2 + 1e-32f);
    };
    const float scGH = sc(G, H);
    int bi = -1;
    float bg = -INFINITY;
    for (int i = 0; i < m - 1; ++i) {
      const bool valid = CL[i] >= (float)ctx.min_data
          && (C - CL[i]) >= (float)ctx.min_data
          && HL[i] >= (float)ctx.min_hess
          && (H - HL[i]) >= (float)ctx.min_hess;
      const float gain = valid
          ? sc(GL[i], HL[i]) + sc(G - GL[i], H - HL[i]) - scGH
          : -INFINITY;
      if (gain > bg) { bg = gain; bi = i; }
    }
    if (bi < 0 || !std::isfinite(bg)) continue;
    if (best.feat < 0 || bg > best.gain) {
      best.gain = bg;
      best.feat = ctx.cat_feats[ci];
      best.GL = GL[bi]; best.HL = HL[bi]; best.CL = CL[bi];
      best.cats.assign(order.begin(), order.begin() + bi + 1);
      for (auto& v : best.cats) v = present[v];
    }
  }
  return best;
}

// Fill a candidate's split from the readbacks: numeric scan row `hi`, then
// let the categorical best take over iff strictly better (trainer._scan).
void resolve_best(const GrowCtx& ctx, SplitJob& job, int hi, LeafCand& c) {
  // arg-max over the per-feature records, by split_reduce_k's rule: highest
  // gain, ties to the lowest feature, all -inf -> feature 0's record
  auto rec = job.scan_host.accessor<float, 3>()[hi];
  long bf = 0;
  float best = -INFINITY;
  for (long f = 0; f < rec.size(0); ++f)
    if (rec[f][0] > best) { best = rec[f][0]; bf = f; }
  auto a = rec[bf];
  c.gain = a[0]; c.feat = (int)a[1]; c.bin = (int)a[2];
  c.GL = a[3]; c.HL = a[4]; c.CL = a[5];
  c.cats.clear();
  if (!ctx.cat_feats.empty()) {
    const size_t stride =
        ctx.cat_feats.size() * (size_t)ctx.n_bins * 3;
    CatBest cb = cat_scan_host(
        ctx, job.cat_host.data_ptr<int64_t>() + (size_t)hi * stride);
    if (cb.feat >= 0 && (double)cb.gain > c.gain) {
      c.gain = (double)cb.gain; c.feat = cb.feat; c.bin = 0;
      c.GL = (double)cb.GL; c.HL = (double)cb.HL; c.CL = (double)cb.CL;
      c.cats = std::move(cb.cats);
    }
  }
}

// Launch a leaf's whole chain (bitset copy, count, scatter, small-child
// histogram, sibling scan, readbacks, event) on the next stream of the pool.
// No device-side wait orders it after other chains, and none is needed: a
// chain is launched only for a leaf whose creating chain's event the host
// has already waited on (the root: the root scan's event, which also covers
// the arena setup), and live leaves own disjoint arena ranges.  That holds
// for a root on the static planes too: its chain reads binned_pair and
// buffer 0's records and row ids over [0, n) and writes buffer 1; buffer 0
// is written again only by chains of the root's children, which start after
// the root chain's event, and binned_pair is never a destination (child_buf
// never returns kRootBuf).  Keep that invariant when changing the loop below.
void launch_job(GrowCtx& ctx, LeafCand& leaf) {
  const size_t si = ctx.next_stream;
  ctx.next_stream = (ctx.next_stream + 1) % ctx.streams.size();
  // grower_stream() and every tensor allocated below belong to this stream
  c10::hip::HIPStreamGuard guard(ctx.streams[si]);
  int* const scratch = ctx.scratch[si].data_ptr<int>();
  int* const total = ctx.total[si].data_ptr<int>();
  auto job = std::make_shared<SplitJob>();
  const long m = leaf.hi - leaf.lo;
  const int src = leaf.buf, dst = child_buf(leaf.buf);
  const unsigned* cat_bits = nullptr;
  if (!leaf.cats.empty()) {
    // categorical split: stage the 256-bit category set and partition by
    // bitset test instead of bin <= thr
    job->bits_host = torch::zeros({8}, torch::TensorOptions()
                                           .dtype(torch::kInt32)
                                           .pinned_memory(true));
    unsigned* wb = (unsigned*)job->bits_host.data_ptr<int>();
    for (int b : leaf.cats) wb[b >> 5] |= (1u << (b & 31));
    job->bits_dev = torch::empty({8}, ctx.rowid[0].options()
                                          .dtype(torch::kInt32));
    (void)hipMemcpyAsync(job->bits_dev.data_ptr<int>(), wb,
                         8 * sizeof(int), hipMemcpyHostToDevice,
                         grower_stream());
    cat_bits = (const unsigned*)job->bits_dev.data_ptr<int>();
  }
  launch_partition_arena(
      pair_of(ctx, src), ctx.ghq[small_buf(src)].data_ptr(),
      ctx.rowid[small_buf(src)].data_ptr<int>(), ctx.pair[dst].data_ptr(),
      ctx.ghq[dst].data_ptr(), ctx.rowid[dst].data_ptr<int>(), ctx.n_arena,
      ctx.npairs, leaf.lo, m, leaf.feat, leaf.bin, cat_bits,
      scratch, total, 0, 0, grower_stream());

  const double CL = leaf.CL, CR = leaf.C - leaf.CL;
  const bool left_small = CL <= CR;  // by GLOBAL counts: same on all ranks
  torch::Tensor hist_small;
  if (!ctx.distributed && leaf.C < 1.6e7) {
    job->nl_known = (long)leaf.CL;  // exact integer counts on this rank
    const long lo_s = left_small ? leaf.lo : leaf.lo + job->nl_known;
    const long m_s = left_small ? job->nl_known : m - job->nl_known;
    hist_small = build_hist(ctx, dst, lo_s, m_s);
  } else {
    hist_small = build_hist(ctx, dst, leaf.lo, m, total, left_small ? 0 : 1);
    job->nl_host = torch::empty({1}, torch::TensorOptions()
                                         .dtype(torch::kInt32)
                                         .pinned_memory(true));
    (void)hipMemcpyAsync(job->nl_host.data_ptr<int>(), total, sizeof(int),
                         hipMemcpyDeviceToHost, grower_stream());
  }
  auto hist_big = hist_slot(ctx, false);
  job->hist_l = left_small ? hist_small : hist_big;
  job->hist_r = left_small ? hist_big : hist_small;
  launch_scan_async(ctx, leaf.hist, hist_small, hist_big, left_small, *job);
  leaf.job = job;
}

double leaf_output(double G, double H, double l1, double l2,
                   double max_delta) {
  double g = std::abs(G) - l1;
  if (g <= 0) return 0.0;
  double denom = H + l2;
  if (denom <= 0) return 0.0;  // all-zero quantized hessians, no L2
  double w = -std::copysign(g, G) / denom;
  if (max_delta > 0) w = std::clamp(w, -max_delta, max_delta);
  return w;
}

bool splittable(const GrowCtx& ctx, const LeafCand& c) {
  if (!(c.gain > ctx.min_gain) || !std::isfinite(c.gain)) return false;
  if (ctx.max_depth > 0 && c.depth >= ctx.max_depth) return false;
  return true;
}

}  // namespace

// Returns dict with node arrays (CPU int32/f32 tensors), per-leaf rows
// (device int32, concatenated) + offsets + leaf node ids, and preds_applied.
// rows_identity promises rows_root[i] == i for all i (every row, in order).
// With preds_col the tree's update, preds_col[row] += (float)((double)leaf
// value * shrinkage), is launched on the caller's stream before returning.
py::dict grow_tree_native(torch::Tensor binned, torch::Tensor binned_pair,
                          torch::Tensor rows_root,
                          torch::Tensor grad, torch::Tensor hess,
                          long n_bins, long nf, double scale_g, double scale_h,
                          double l1, double l2, double min_data,
                          double min_hess, double min_gain, double max_delta,
                          long num_leaves, long max_depth,
                          c10::optional<torch::Tensor> feat_mask,
                          c10::optional<torch::Tensor> cat_feats,
                          double cat_smooth,
                          py::object process_group, bool distributed,
                          bool rows_identity,
                          c10::optional<torch::Tensor> preds_col,
                          double shrinkage) {
  GrowCtx ctx;
  const long n_full = binned_pair.size(1);
  ctx.n_arena = rows_root.numel();
  // rows_identity: rows_root[i] == i for every i, so buffer 0's planes would
  // be a copy of binned_pair and the root reads binned_pair instead
  const bool root_static =
      grower_switch("MMLSPARK_AMD_GROWER_ROOT_STATIC") && rows_identity;
  const bool root_one_wait = grower_switch("MMLSPARK_AMD_GROWER_ROOT_ONE_WAIT");
  const bool apply_here =
      grower_switch("MMLSPARK_AMD_GROWER_APPLY") && preds_col.has_value();
  if (rows_identity)
    TORCH_CHECK(ctx.n_arena == n_full && binned_pair.is_contiguous() &&
                binned_pair.scalar_type() == torch::kInt64,
                "rows_identity needs rows_root to be all ", n_full,
                " rows and contiguous i64 bin planes, got ", ctx.n_arena,
                " rows");
  if (preds_col.has_value())
    TORCH_CHECK(preds_col->is_cuda() && preds_col->dim() == 1 &&
                preds_col->scalar_type() == torch::kFloat32 &&
                preds_col->size(0) >= n_full,
                "preds_col: 1-D f32 device tensor over all rows");
  ctx.n_bins = (int)n_bins;
  ctx.npairs = (int)binned_pair.size(0);
  ctx.tail_bytes = (int)(binned.size(0) * 4 - (ctx.npairs - 1) * 8);
  ctx.nf = nf;
  ctx.scale_g = scale_g;
  ctx.scale_h = scale_h;
  ctx.l1 = l1; ctx.l2 = l2;
  ctx.min_data = min_data; ctx.min_hess = min_hess; ctx.min_gain = min_gain;
  ctx.num_leaves = (int)num_leaves;
  ctx.max_depth = (int)max_depth;
  if (feat_mask.has_value()) ctx.feat_mask = *feat_mask;
  if (cat_feats.has_value() && cat_feats->numel() > 0) {
    auto cf = cat_feats->to(torch::kInt64).contiguous().cpu();
    auto acc = cf.accessor<int64_t, 1>();
    for (long i = 0; i < cf.numel(); ++i)
      ctx.cat_feats.push_back((int)acc[i]);
    ctx.cat_idx_dev = cf.to(binned.device());
    ctx.cat_smooth = cat_smooth;
  }
  if (!process_group.is_none()) {
    ctx.pg = process_group.cast<c10::intrusive_ptr<c10d::ProcessGroup>>();
  }
  ctx.has_reduce = ctx.pg && ctx.pg->getSize() > 1;
  ctx.distributed = distributed;
  // a real process group stays on one stream: the order of collectives
  // across streams would have to match on every rank
  ctx.streams = grower_streams(ctx.has_reduce ? 1 : grower_streams_from_env());
  // a bad histogram setting raises here, before any chain is in flight
  (void)hist_threads();
  (void)hist_order();
  (void)hist_layout();

  py::gil_scoped_release nogil;

  for (size_t s = 0; s < ctx.streams.size(); ++s) {
    ctx.scratch[s] =
        torch::empty({4096}, rows_root.options().dtype(torch::kInt32));
    ctx.total[s] = torch::zeros({1}, rows_root.options().dtype(torch::kInt32));
  }
  auto i64d = rows_root.options().dtype(torch::kInt64);
  // one zero fill per tree instead of one per split: root + one small child
  // per split, with room for the two speculated chains
  // (slabs capped at 1 GiB each; hist_slot allocates per split beyond that)
  const long slot_bytes = (long)ctx.npairs * 8 * ctx.n_bins * 3 * 8;
  const long slots = std::min<long>(ctx.num_leaves + 2,
                                    std::max<long>(1, (1l << 30) / slot_bytes));
  ctx.slab_zero = torch::zeros({slots, ctx.npairs * 8, ctx.n_bins, 3}, i64d);
  ctx.slab_raw = torch::empty({slots, ctx.npairs * 8, ctx.n_bins, 3}, i64d);
  for (int b = 0; b < 2; ++b) {
    ctx.pair[b] = torch::empty({ctx.npairs, ctx.n_arena}, i64d);
    ctx.ghq[b] = torch::empty({ctx.n_arena, 2}, i64d);
    ctx.rowid[b] = torch::empty({ctx.n_arena},
                                rows_root.options().dtype(torch::kInt32));
  }
  // materialize arena buffer 0: bin pairs + quantized (gq,hq) + row ids for
  // the (possibly bagged) root row set; with the root on the static planes
  // no plane is copied (zero planes) and pair[0] is first written by the
  // root's grandchildren
  if (root_static) ctx.root_pair = binned_pair.data_ptr();
  launch_arena_gather(binned_pair.data_ptr(), n_full,
                      grad.data_ptr<float>(), hess.data_ptr<float>(),
                      rows_root.data_ptr<int>(), ctx.n_arena,
                      root_static ? 0 : ctx.npairs,
                      ctx.scale_g, ctx.scale_h, ctx.pair[0].data_ptr(),
                      ctx.ghq[0].data_ptr(), ctx.rowid[0].data_ptr<int>(),
                      grower_stream());

  std::vector<int> feature_, thr_bin_, left_, right_, leaf_idx_;
  std::vector<int> cat_off_, cat_words_;
  std::vector<float> value_, count_, gain_;
  auto new_node = [&]() {
    feature_.push_back(-1); thr_bin_.push_back(0); left_.push_back(-1);
    right_.push_back(-1); value_.push_back(0.f); count_.push_back(0.f);
    gain_.push_back(0.f); leaf_idx_.push_back(-1); cat_off_.push_back(-1);
    return (int)feature_.size() - 1;
  };

  const int root_buf = root_static ? kRootBuf : 0;
  auto root_hist = build_hist(ctx, root_buf, 0, ctx.n_arena);
  auto root = std::make_shared<LeafCand>();
  root->node_id = new_node();
  root->lo = 0; root->hi = ctx.n_arena; root->buf = root_buf;
  root->hist = root_hist;
  // root totals = feature 0's histogram row summed over its bins, in int64
  int64_t s0[3] = {0, 0, 0};
  if (root_one_wait) {
    // the row rides back behind the same event as the root scan's records
    // and is summed on the host: exact, so equal to a device reduction
    SplitJob j;
    launch_scan_async(ctx, torch::Tensor(), root_hist, torch::Tensor(), true,
                      j, /*row0=*/true);
    (void)hipEventSynchronize(j.ev);
    const int64_t* r = j.row0_host.data_ptr<int64_t>();
    for (int b = 0; b < ctx.n_bins; ++b)
      for (int c = 0; c < 3; ++c) s0[c] += r[b * 3 + c];
    resolve_best(ctx, j, 0, *root);
  } else {
    auto sums = root_hist.select(0, 0).sum(0).to(torch::kCPU);
    auto sa = sums.accessor<int64_t, 1>();
    for (int c = 0; c < 3; ++c) s0[c] = sa[c];
    // one-time root scan through the same async machinery
    SplitJob j;
    launch_scan_async(ctx, torch::Tensor(), root_hist, torch::Tensor(), true,
                      j);
    (void)hipEventSynchronize(j.ev);
    resolve_best(ctx, j, 0, *root);
  }
  const double G0 = (double)s0[0] / scale_g;
  const double H0 = (double)s0[1] / scale_h;
  const double C0 = (double)s0[2];
  root->G = G0; root->H = H0; root->C = C0;
  count_[root->node_id] = (float)C0;
  value_[root->node_id] = (float)leaf_output(G0, H0, l1, l2, max_delta);

  std::priority_queue<CandPtr, std::vector<CandPtr>, CandCmp> heap;
  std::vector<CandPtr> finals;
  heap.push(root);
  finals.push_back(root);
  long seq = 1;
  int n_leaves = 1;

  while (n_leaves < ctx.num_leaves && !heap.empty()) {
    CandPtr leaf = heap.top();
    heap.pop();
    if (!splittable(ctx, *leaf)) continue;
    for (size_t i = 0; i < finals.size(); ++i)
      if (finals[i]->node_id == leaf->node_id) {
        finals.erase(finals.begin() + i);
        break;
      }

    if (!leaf->job) launch_job(ctx, *leaf);
    // speculate: pre-launch the next-best candidate's chain so its GPU work
    // overlaps this readback (exact commit order preserved; the cache is
    // consumed whenever that leaf is popped; live leaves own disjoint row
    // ranges so in-flight scatters never collide)
    if (n_leaves + 1 < ctx.num_leaves && !heap.empty()) {
      CandPtr nxt = heap.top();
      if (!nxt->job && splittable(ctx, *nxt)) launch_job(ctx, *nxt);
      if (n_leaves + 2 < ctx.num_leaves && heap.size() >= 2) {
        heap.pop();  // peek the second-best, then restore
        CandPtr nxt2 = heap.top();
        heap.push(nxt);
        if (!nxt2->job && splittable(ctx, *nxt2)) launch_job(ctx, *nxt2);
      }
    }

    SplitJob& job = *leaf->job;
    (void)hipEventSynchronize(job.ev);
    const long m_parent = leaf->hi - leaf->lo;
    const long nl = job.nl_known >= 0
                        ? job.nl_known
                        : (long)job.nl_host.data_ptr<int>()[0];

    const double GL = leaf->GL, HL = leaf->HL, CL = leaf->CL;
    const double GR = leaf->G - GL, HR = leaf->H - HL, CR = leaf->C - CL;
    const int nid = leaf->node_id;
    feature_[nid] = leaf->feat;
    thr_bin_[nid] = leaf->bin;
    gain_[nid] = (float)leaf->gain;
    if (!leaf->cats.empty()) {
      unsigned words[8] = {0};
      for (int b : leaf->cats) words[b >> 5] |= (1u << (b & 31));
      cat_off_[nid] = (int)(cat_words_.size() / 8);
      for (int w = 0; w < 8; ++w) cat_words_.push_back((int)words[w]);
    }
    const int lid = new_node();
    const int rid = new_node();
    left_[nid] = lid;
    right_[nid] = rid;
    count_[lid] = (float)CL;
    count_[rid] = (float)CR;
    value_[lid] = (float)leaf_output(GL, HL, l1, l2, max_delta);
    value_[rid] = (float)leaf_output(GR, HR, l1, l2, max_delta);

    auto lc = std::make_shared<LeafCand>();
    auto rc = std::make_shared<LeafCand>();
    lc->node_id = lid; rc->node_id = rid;
    lc->depth = rc->depth = leaf->depth + 1;
    lc->buf = rc->buf = child_buf(leaf->buf);
    lc->lo = leaf->lo; lc->hi = leaf->lo + nl;
    rc->lo = leaf->lo + nl; rc->hi = leaf->lo + m_parent;
    lc->hist = job.hist_l; rc->hist = job.hist_r;
    lc->G = GL; lc->H = HL; lc->C = CL;
    rc->G = GR; rc->H = HR; rc->C = CR;
    resolve_best(ctx, job, 0, *lc);
    resolve_best(ctx, job, 1, *rc);
    lc->seq = seq++;
    rc->seq = seq++;
    leaf->job.reset();
    leaf->hist = torch::Tensor();  // free parent histogram
    heap.push(lc);
    heap.push(rc);
    finals.push_back(lc);
    finals.push_back(rc);
    n_leaves += 1;
  }

  // The caller's stream joins every side stream before it reads the row-id
  // segments and before the arena, the slabs and the counters (all allocated
  // on the caller's stream) are released: chains that were speculated but
  // never committed may still be writing them.
  for (size_t s = 1; s < ctx.streams.size(); ++s) {
    hipEvent_t ev = nullptr;
    (void)hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    (void)hipEventRecord(ev, ctx.streams[s].stream());
    (void)hipStreamWaitEvent(grower_stream(), ev, 0);
    (void)hipEventDestroy(ev);
  }

  // leaf ordinals in node order; collect original-row-id segments from each
  // leaf's own arena buffer
  std::sort(finals.begin(), finals.end(),
            [](const CandPtr& a, const CandPtr& b) {
              return a->node_id < b->node_id;
            });
  std::vector<torch::Tensor> segs;
  std::vector<int64_t> seg_nodes;
  for (size_t i = 0; i < finals.size(); ++i) {
    leaf_idx_[finals[i]->node_id] = (int)i;
    segs.push_back(ctx.rowid[small_buf(finals[i]->buf)].slice(
        0, finals[i]->lo, finals[i]->hi));
    seg_nodes.push_back(finals[i]->node_id);
  }
  auto leaf_rows = segs.empty()
                       ? torch::empty({0}, rows_root.options())
                       : torch::cat(segs);
  std::vector<int64_t> offs(1, 0);
  for (auto& s : segs) offs.push_back(offs.back() + s.numel());

  // prediction update, launched here so that it runs while the caller builds
  // its tree object: preds_col[row] += (float)(leaf value * shrinkage).  The
  // offsets and values go up from pinned tensors without blocking; torch's
  // host allocator keeps them alive until the copies are done.
  const bool applied = apply_here && leaf_rows.numel() > 0;
  if (applied) {
    const long nl = (long)segs.size();
    auto pin = torch::TensorOptions().pinned_memory(true);
    auto offs_h = torch::empty({nl + 1}, pin.dtype(torch::kInt64));
    auto vals_h = torch::empty({nl}, pin.dtype(torch::kFloat32));
    std::copy(offs.begin(), offs.end(), offs_h.data_ptr<int64_t>());
    for (long i = 0; i < nl; ++i)
      vals_h.data_ptr<float>()[i] =
          (float)((double)value_[seg_nodes[i]] * shrinkage);
    auto offs_d = offs_h.to(leaf_rows.device(), /*non_blocking=*/true);
    auto vals_d = vals_h.to(leaf_rows.device(), /*non_blocking=*/true);
    launch_apply_leaf_values(preds_col->data_ptr<float>(),
                             preds_col->stride(0), leaf_rows.data_ptr<int>(),
                             (const long*)offs_d.data_ptr<int64_t>(), (int)nl,
                             vals_d.data_ptr<float>(), leaf_rows.numel(),
                             grower_stream());
  }

  py::gil_scoped_acquire gil;
  auto i32 = torch::TensorOptions().dtype(torch::kInt32);
  auto f32 = torch::TensorOptions().dtype(torch::kFloat32);
  py::dict d;
  d["feature"] = torch::tensor(feature_, i32);
  d["thr_bin"] = torch::tensor(thr_bin_, i32);
  d["left"] = torch::tensor(left_, i32);
  d["right"] = torch::tensor(right_, i32);
  d["value"] = torch::tensor(value_, f32);
  d["count"] = torch::tensor(count_, f32);
  d["gain"] = torch::tensor(gain_, f32);
  d["leaf_index"] = torch::tensor(leaf_idx_, i32);
  d["leaf_rows"] = leaf_rows;
  d["leaf_offsets"] = torch::tensor(offs, torch::kInt64);
  d["leaf_nodes"] = torch::tensor(seg_nodes, torch::kInt64);
  d["cat_offset"] = torch::tensor(cat_off_, i32);
  d["cat_words"] = cat_words_.empty()
                       ? torch::zeros({0}, i32)
                       : torch::tensor(cat_words_, i32);
  // (1,) i32: 1 iff preds_col already holds this tree's update
  d["preds_applied"] = torch::full({1}, applied ? 1 : 0, i32);
  return d;
}

// Standalone C++ c10d all_reduce — lets the gloo world_size=2 CPU tests
// prove the exact binding the grower uses (pg cast + allreduce + wait)
// without a GPU, and gives other native paths a GIL-free reduce.
void allreduce_native(py::object process_group, torch::Tensor t) {
  auto pg = process_group.cast<c10::intrusive_ptr<c10d::ProcessGroup>>();
  py::gil_scoped_release nogil;
  std::vector<at::Tensor> v{t};
  pg->allreduce(v)->wait();
}

// preds_col[leaf_rows[i]] += values[leaf of i] in one launch; preds_col may be
// a strided column view.  leaf_offsets: (n_leaves + 1,) i64, any device.
void apply_leaf_values(torch::Tensor preds_col, torch::Tensor leaf_rows,
                       torch::Tensor leaf_offsets, torch::Tensor values) {
  TORCH_CHECK(preds_col.is_cuda() && preds_col.dim() == 1 &&
              preds_col.scalar_type() == torch::kFloat32,
              "preds_col: 1-D f32 device tensor");
  TORCH_CHECK(leaf_rows.is_cuda() && leaf_rows.is_contiguous() &&
              leaf_rows.scalar_type() == torch::kInt32,
              "leaf_rows: contiguous i32 device tensor");
  TORCH_CHECK(values.is_cuda() && values.is_contiguous() &&
              values.scalar_type() == torch::kFloat32,
              "values: contiguous f32 device tensor");
  TORCH_CHECK(leaf_offsets.scalar_type() == torch::kInt64 &&
              leaf_offsets.numel() == values.numel() + 1,
              "leaf_offsets: i64 of n_leaves + 1");
  auto offs_cpu = leaf_offsets.cpu();
  const int64_t* oc = offs_cpu.data_ptr<int64_t>();
  const long n_leaves = values.numel();
  TORCH_CHECK(oc[0] == 0 && oc[n_leaves] == leaf_rows.numel(),
              "leaf_offsets must span leaf_rows");
  for (long l = 0; l < n_leaves; ++l)
    TORCH_CHECK(oc[l] <= oc[l + 1], "leaf_offsets must be non-decreasing");
  auto offs = leaf_offsets.to(preds_col.device()).contiguous();
  launch_apply_leaf_values(preds_col.data_ptr<float>(), preds_col.stride(0),
                           leaf_rows.data_ptr<int>(),
                           (const long*)offs.data_ptr<int64_t>(),
                           (int)n_leaves, values.data_ptr<float>(),
                           leaf_rows.numel(), grower_stream());
}

// Test/tuning entry for the arena partition: scatters rows [lo, lo+m) of the
// src arena into dst (stable left|right) and returns the device left count.
// chunk / plane_groups = 0 take the launcher's own policy.
torch::Tensor partition_arena(torch::Tensor pair_src, torch::Tensor ghq_src,
                              torch::Tensor rowid_src, torch::Tensor pair_dst,
                              torch::Tensor ghq_dst, torch::Tensor rowid_dst,
                              long lo, long m, long feature, long thr,
                              c10::optional<torch::Tensor> cat_bits,
                              long chunk, long plane_groups) {
  const long n_arena = pair_src.size(1);
  const long npairs = pair_src.size(0);
  TORCH_CHECK(pair_src.is_cuda() && pair_src.is_contiguous() &&
              pair_src.scalar_type() == torch::kInt64 &&
              pair_dst.is_contiguous() && pair_dst.sizes() == pair_src.sizes(),
              "pair planes: contiguous (npairs, n_arena) i64");
  TORCH_CHECK(ghq_src.is_contiguous() && ghq_dst.is_contiguous() &&
              ghq_src.numel() == 2 * n_arena && ghq_dst.numel() == 2 * n_arena,
              "ghq: contiguous (n_arena, 2) i64");
  TORCH_CHECK(rowid_src.is_contiguous() && rowid_dst.is_contiguous() &&
              rowid_src.numel() == n_arena && rowid_dst.numel() == n_arena,
              "rowid: contiguous (n_arena,) i32");
  TORCH_CHECK(lo >= 0 && m >= 0 && lo + m <= n_arena, "range out of bounds");
  TORCH_CHECK(feature >= 0 && feature < npairs * 8, "feature out of range");
  const unsigned* bits = nullptr;
  if (cat_bits.has_value()) {
    TORCH_CHECK(cat_bits->is_cuda() && cat_bits->is_contiguous() &&
                cat_bits->scalar_type() == torch::kInt32 &&
                cat_bits->numel() == 8, "cat_bits: (8,) i32 device");
    bits = (const unsigned*)cat_bits->data_ptr<int>();
  }
  auto i32 = rowid_src.options().dtype(torch::kInt32);
  auto scratch = torch::empty({4096}, i32);
  auto total = torch::zeros({1}, i32);
  launch_partition_arena(pair_src.data_ptr(), ghq_src.data_ptr(),
                         rowid_src.data_ptr<int>(), pair_dst.data_ptr(),
                         ghq_dst.data_ptr(), rowid_dst.data_ptr<int>(),
                         n_arena, (int)npairs, lo, m, (int)feature, (int)thr,
                         bits, scratch.data_ptr<int>(), total.data_ptr<int>(),
                         chunk, (int)plane_groups, grower_stream());
  return total;
}

// Test/tuning entry for the range-mode histogram: adds the (g, h, count)
// sums of arena rows [lo, lo+m) into `hist` (nf_pad, n_bins, 3).  With side
// 0 / 1 only the left / right part of the range is read, split at the device
// count nl_dev[0], which the caller keeps within [0, m], as it keeps every
// bin byte of the valid features below n_bins: neither can be checked here
// without reading the arena back.  chunk = 0, threads = 0, order = -1 and
// layout = -1 take the environment's setting if there is one and else the
// launcher's policy.
void hist_pair_range(torch::Tensor pair, torch::Tensor ghq, long lo, long m,
                     torch::Tensor hist, long n_bins, long tail_bytes,
                     c10::optional<torch::Tensor> nl_dev, long side,
                     long chunk, long threads, long order, long layout) {
  TORCH_CHECK(pair.is_cuda() && pair.is_contiguous() && pair.dim() == 2 &&
              pair.scalar_type() == torch::kInt64,
              "pair planes: contiguous (npairs, n_arena) i64");
  const long n_arena = pair.size(1);
  const long npairs = pair.size(0);
  TORCH_CHECK(ghq.is_cuda() && ghq.is_contiguous() &&
              ghq.scalar_type() == torch::kInt64 &&
              ghq.numel() == 2 * n_arena,
              "ghq: contiguous (n_arena, 2) i64");
  TORCH_CHECK(lo >= 0 && m >= 0 && lo + m <= n_arena, "range out of bounds");
  TORCH_CHECK(n_bins >= 1 && n_bins <= 256, "n_bins must be 1..256");
  TORCH_CHECK(tail_bytes >= 1 && tail_bytes <= 8, "tail_bytes must be 1..8");
  TORCH_CHECK(hist.is_cuda() && hist.is_contiguous() &&
              hist.scalar_type() == torch::kInt64 &&
              hist.numel() == npairs * 8 * n_bins * 3,
              "hist: contiguous (npairs * 8, n_bins, 3) i64");
  TORCH_CHECK(side >= -1 && side <= 1, "side must be -1, 0 or 1");
  TORCH_CHECK(chunk >= 0, "chunk must be >= 0");
  const int threads_r = hist_threads(threads);
  const int order_r = hist_order(order);
  const int layout_r = hist_layout(layout);
  const int* nl = nullptr;
  if (side >= 0) {
    TORCH_CHECK(nl_dev.has_value() && nl_dev->is_cuda() &&
                nl_dev->scalar_type() == torch::kInt32 &&
                nl_dev->numel() == 1, "nl_dev: (1,) i32 device");
    nl = nl_dev->data_ptr<int>();
  }
  launch_hist_pair_range(pair.data_ptr(), ghq.data_ptr(), n_arena, lo, m,
                         (long long*)hist.data_ptr<int64_t>(), (int)n_bins,
                         (int)npairs, (int)tail_bytes, nl, (int)side, chunk,
                         threads_r, order_r, layout_r, grower_stream());
}

// Test entry for the fused sibling subtract + scan (sibling_scan_k), the
// kernel launch_scan_async issues: `small` (nf_pad, n_bins, 3) int64 is one
// child's fixed-point histogram as built; with `parent` the other child's is
// formed as parent - small, stored into a fresh `big` and scanned in the same
// launch (record row 0 = left child, row 1 = right child); without it `small`
// is scanned alone (the root) and big is None.  Returns the per-feature
// records (nh, nf_pad, 6) = {gain, feature, bin, GL, HL, CL}; the arg-max over
// features is the caller's.  scale_g / scale_h are the fixed-point scales of
// the g and h cells.  Everything the kernel indexes with is checked here.
std::tuple<torch::Tensor, c10::optional<torch::Tensor>> sibling_scan(
    c10::optional<torch::Tensor> parent, torch::Tensor small,
    bool small_is_left, long n_bins, double l1, double l2, double min_data,
    double min_hess, long nf_real, c10::optional<torch::Tensor> feat_mask,
    double scale_g, double scale_h) {
  TORCH_CHECK(small.is_cuda() && small.is_contiguous() && small.dim() == 3 &&
              small.scalar_type() == torch::kInt64 && small.size(2) == 3,
              "small: contiguous (nf_pad, n_bins, 3) i64 device");
  // one 256-thread block scans a feature: a bin per thread, 256 LDS slots
  TORCH_CHECK(n_bins >= 2 && n_bins <= 256, "n_bins must be in 2..256");
  TORCH_CHECK(small.size(1) == n_bins, "n_bins must equal small.size(1)");
  const long nf_pad = small.size(0);
  TORCH_CHECK(nf_real > 0 && nf_real <= nf_pad,
              "nf_real must be in 1..nf_pad");
  TORCH_CHECK(scale_g > 0 && scale_h > 0, "scales must be positive");
  const long long* parent_ptr = nullptr;
  if (parent.has_value()) {
    TORCH_CHECK(parent->device() == small.device() &&
                parent->is_contiguous() &&
                parent->scalar_type() == torch::kInt64 &&
                parent->sizes() == small.sizes(),
                "parent: contiguous i64 of small's shape and device");
    parent_ptr = (const long long*)parent->data_ptr<int64_t>();
  }
  const bool* mask = nullptr;
  if (feat_mask.has_value()) {
    TORCH_CHECK(feat_mask->device() == small.device(),
                "feat_mask must live where small lives");
    TORCH_CHECK(feat_mask->scalar_type() == torch::kBool,
                "feat_mask must be bool");
    TORCH_CHECK(feat_mask->is_contiguous() && feat_mask->numel() >= nf_pad,
                "feat_mask must be contiguous with at least nf_pad elements");
    mask = feat_mask->data_ptr<bool>();
  }
  const long nh = parent_ptr ? 2 : 1;
  auto records = torch::empty(
      {nh, nf_pad, 6},
      torch::TensorOptions().dtype(torch::kFloat32).device(small.device()));
  c10::optional<torch::Tensor> big;
  if (parent_ptr) big = torch::empty_like(small);
  launch_sibling_scan(
      parent_ptr, (const long long*)small.data_ptr<int64_t>(),
      big.has_value() ? (long long*)big->data_ptr<int64_t>() : nullptr,
      small_is_left ? 1 : 0, nf_pad, (int)n_bins, (float)l1, (float)l2,
      (float)min_data, (float)min_hess, nf_real, mask,
      records.data_ptr<float>(), 1.0 / scale_g, 1.0 / scale_h,
      grower_stream());
  return {records, big};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("grow_tree_native", &grow_tree_native,
        "native leaf-wise GBDT tree growth (arena mode)", py::arg("binned"),
        py::arg("binned_pair"), py::arg("rows_root"), py::arg("grad"),
        py::arg("hess"), py::arg("n_bins"), py::arg("nf"), py::arg("scale_g"),
        py::arg("scale_h"), py::arg("l1"), py::arg("l2"), py::arg("min_data"),
        py::arg("min_hess"), py::arg("min_gain"), py::arg("max_delta"),
        py::arg("num_leaves"), py::arg("max_depth"), py::arg("feat_mask"),
        py::arg("cat_feats"), py::arg("cat_smooth"), py::arg("process_group"),
        py::arg("distributed"), py::arg("rows_identity") = false,
        py::arg("preds_col") = py::none(), py::arg("shrinkage") = 1.0);
  m.def("apply_leaf_values", &apply_leaf_values,
        "preds_col[leaf_rows] += per-leaf value, one kernel");
  m.def("partition_arena", &partition_arena,
        "arena stable partition (count + fused scatter)", py::arg("pair_src"),
        py::arg("ghq_src"), py::arg("rowid_src"), py::arg("pair_dst"),
        py::arg("ghq_dst"), py::arg("rowid_dst"), py::arg("lo"), py::arg("m"),
        py::arg("feature"), py::arg("thr"), py::arg("cat_bits") = py::none(),
        py::arg("chunk") = 0, py::arg("plane_groups") = 0);
  m.def("hist_pair_range", &hist_pair_range,
        "range-mode arena histogram, accumulated into hist", py::arg("pair"),
        py::arg("ghq"), py::arg("lo"), py::arg("m"), py::arg("hist"),
        py::arg("n_bins"), py::arg("tail_bytes"),
        py::arg("nl_dev") = py::none(), py::arg("side") = -1,
        py::arg("chunk") = 0, py::arg("threads") = 0, py::arg("order") = -1,
        py::arg("layout") = -1);
  m.def("sibling_scan", &sibling_scan,
        "fused sibling subtract + per-feature split scan (records, big)",
        py::arg("parent"), py::arg("small"), py::arg("small_is_left"),
        py::arg("n_bins"), py::arg("l1"), py::arg("l2"), py::arg("min_data"),
        py::arg("min_hess"), py::arg("nf_real"),
        py::arg("feat_mask") = py::none(), py::arg("scale_g") = 1.0,
        py::arg("scale_h") = 1.0);
  m.def("allreduce_native", &allreduce_native,
        "GIL-free c10d all_reduce through the same C++ path as the grower");
}
