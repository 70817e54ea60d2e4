// Exact k-nearest-neighbour search for MI355X (gfx950): fused distance +
// selection, no (n_queries, n_index) tile in memory.
//
//   knn_partial_topk_k  grid = query tiles x index splits.  A workgroup of
//       four waves takes KNN_TQ = 128 queries and one contiguous split of the
//       index, walks the split in tiles of KNN_TN = 128 points and forms the
//       dot products with v_mfma_f32_32x32x2_f32 from operands staged in LDS:
//       index points on the rows (A), queries on the columns (B), so the 64
//       accumulators of a lane (4 row tiles x 16) all belong to ONE query and
//       that query's threshold lives in two registers.  In the accumulators
//       s = xsq[j] - 2*dot (||q||^2 does not change a query's order and is
//       added by the merge).  Per query a sorted list of the k best (s, index)
//       pairs is kept in LDS under the total order (s ascending, index
//       ascending); its last entry is the threshold.  Lanes filter their
//       accumulators against the threshold; the few survivors are checked
//       against the query's label bitset and pushed into a per-query bounded
//       queue (an LDS counter per query); after a barrier the query's owner
//       thread drains the queue into the list.  Lanes that found the queue
//       full keep a pending bit per accumulator and retry after the drain,
//       looping on __syncthreads_or: every round either pushes a lane's
//       candidate or drains a full queue of others, so the number of pending
//       candidates falls strictly and nothing is dropped.
//   knn_merge_k  one workgroup per query merges the splits' sorted lists by
//       rank (an element's place is its own position plus, for every other
//       split, the number of elements ahead of it) and writes s + ||q||^2.
//
// The MFMA result is bit-for-bit the k-ordered fmaf chain over the feature
// index, started from 0, whatever tile or split a pair falls into; the order
// is total (indices are distinct).  So the output is the same for every
// number of splits and from call to call.
#include <hip/hip_runtime.h>

#define KNN_TQ 128      // queries per workgroup (4 waves x 32 columns)
#define KNN_TN 128      // index points per tile (4 row tiles of 32)
#define KNN_KC 32       // features staged per chunk
#define KNN_LD 33       // LDS row stride in floats: odd, so conflict-free
#define KNN_QCAP 16     // queue entries per query per round
#define KNN_MAX_K 64
#define KNN_MAX_SPLITS 64

typedef float f32x16 __attribute__((ext_vector_type(16)));

// (s, i) strictly ahead of (ts, ti) in the total order.  A masked or padded
// candidate has s = +inf and is never ahead of anything, (+inf, -1) included:
// a padded row's index may wrap negative when n is within a tile of 2^31, so
// negative indices lose every tie.
__device__ __forceinline__ bool knn_ahead(float s, int i, float ts, int ti) {
  return s < ts || (s == ts && i < ti && i >= 0);
}

// LDS image (dynamic, floats): [Xs TN*LD | Qs TQ*LD | xsq TN | lab TN |
// qcnt TQ | list_s k*TQ | list_i k*TQ].  The queue aliases Xs: it is live only
// between a tile's last MFMA and the next tile's staging, with barriers on
// both sides.  Lists and queue are stored [slot][query], so the 128 owner
// threads touch consecutive banks.
extern "C" __global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(3, 3))) void knn_partial_topk_k(
    const float* __restrict__ Q, const float* __restrict__ X,
    const float* __restrict__ xsq, const int* __restrict__ label_ids,
    const unsigned* __restrict__ allow_bits, long n_q, int n, int d, int k,
    int W, int splits, int tiles_per_split, float* __restrict__ part_s,
    int* __restrict__ part_i) {
  extern __shared__ __attribute__((aligned(16))) float knn_lds[];
  float* Xs = knn_lds;
  float* Qs = Xs + KNN_TN * KNN_LD;
  float* xsq_s = Qs + KNN_TQ * KNN_LD;
  int* lab_s = (int*)(xsq_s + KNN_TN);
  int* qcnt = lab_s + KNN_TN;
  float* list_s = (float*)(qcnt + KNN_TQ);
  int* list_i = (int*)(list_s + (size_t)k * KNN_TQ);
  float* queue_s = Xs;
  int* queue_i = (int*)(Xs + KNN_QCAP * KNN_TQ);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int col = lane & 31;
  const int h = lane >> 5;
  const int ql = wave * 32 + col;             // this lane's query in the tile
  const long qtile = blockIdx.x / splits;
  const int split = (int)(blockIdx.x - qtile * splits);
  const long q0 = qtile * KNN_TQ;
  const long qg = q0 + ql;

  // a query past the end gets a list of (-inf, -1): nothing is ahead of it
  for (int e = tid; e < k * KNN_TQ; e += 256) {
    const bool live = q0 + (e & (KNN_TQ - 1)) < n_q;
    list_s[e] = live ? __builtin_inff() : -__builtin_inff();
    list_i[e] = -1;
  }
  if (tid < KNN_TQ) qcnt[tid] = 0;
  __syncthreads();
  float thr_s = list_s[(k - 1) * KNN_TQ + ql];
  int thr_i = list_i[(k - 1) * KNN_TQ + ql];

  const long n_tiles = ((long)n + KNN_TN - 1) / KNN_TN;
  const long tile_lo = (long)split * tiles_per_split;
  long tile_hi = tile_lo + tiles_per_split;
  if (tile_hi > n_tiles) tile_hi = n_tiles;

  const int skk = tid & 31;   // staging: feature inside the chunk
  const int sp0 = tid >> 5;   // staging: first row, then every 8th

  for (long tile = tile_lo; tile < tile_hi; ++tile) {
    const int base = (int)(tile * KNN_TN);
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int k0 = 0; k0 < d; k0 += KNN_KC) {
      __syncthreads();
      const int kk = k0 + skk;
#pragma unroll 4
      for (int i = 0; i < KNN_TN / 8; ++i) {
        const int p = sp0 + 8 * i;
        const long xr = (long)base + p;
        const long qr = q0 + p;
        Xs[p * KNN_LD + skk] = (xr < n && kk < d) ? X[xr * d + kk] : 0.f;
        Qs[p * KNN_LD + skk] = (qr < n_q && kk < d) ? Q[qr * d + kk] : 0.f;
      }
      if (k0 == 0 && tid < KNN_TN) {
        const long xr = (long)base + tid;
        xsq_s[tid] = xr < n ? xsq[xr] : __builtin_inff();
        lab_s[tid] = (label_ids != nullptr && xr < n) ? label_ids[xr] : 0;
      }
      __syncthreads();
      int steps = (d - k0 + 1) >> 1;
      if (steps > KNN_KC / 2) steps = KNN_KC / 2;
      const float* qrow = Qs + ql * KNN_LD + h;
      const float* xrow = Xs + col * KNN_LD + h;
#pragma unroll 1
      for (int st = 0; st < steps; ++st) {
        const float b = qrow[2 * st];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float a = xrow[t * 32 * KNN_LD + 2 * st];
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
        }
      }
    }

    // s = xsq - 2 dot, kept in the accumulator; one pending bit per survivor
    unsigned pend[4] = {0u, 0u, 0u, 0u};   // one 16-bit mask per row tile
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int pl = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float s = __builtin_fmaf(-2.f, acc[t][r], xsq_s[pl]);
        acc[t][r] = s;
        if (knn_ahead(s, base + pl, thr_s, thr_i))
          pend[t] |= 1u << r;
      }

    while (__syncthreads_or((pend[0] | pend[1] | pend[2] | pend[3]) != 0u)) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const unsigned bit = 1u << r;
          if (pend[t] & bit) {
            const int pc = t * 32 + (r & 3) + 8 * (r >> 2);
            const float s = acc[t][r];
            // opaque, or 64 loop-invariant copies of pl and idx get hoisted
            // out of the retry loop into registers
            int h4 = 4 * h;
            asm volatile("" : "+v"(h4));
            const int pl = pc + h4;
            const int idx = base + pl;
            bool keep = knn_ahead(s, idx, thr_s, thr_i);
            if (keep && label_ids != nullptr) {
              const unsigned lid = (unsigned)lab_s[pl];
              unsigned wi = lid >> 5;
              if (wi > (unsigned)(W - 1)) wi = (unsigned)(W - 1);
              keep = (allow_bits[qg * W + wi] >> (lid & 31u)) & 1u;
            }
            if (keep) {
              const int slot = atomicAdd(&qcnt[ql], 1);
              if (slot < KNN_QCAP) {
                queue_s[slot * KNN_TQ + ql] = s;
                queue_i[slot * KNN_TQ + ql] = idx;
                pend[t] &= ~bit;
              }
            } else {
              pend[t] &= ~bit;
            }
          }
        }
      __syncthreads();
      if (tid < KNN_TQ) {
        int c = qcnt[tid];
        if (c > KNN_QCAP) c = KNN_QCAP;
        qcnt[tid] = 0;
        for (int e = 0; e < c; ++e) {
          const float s = queue_s[e * KNN_TQ + tid];
          const int idx = queue_i[e * KNN_TQ + tid];
          int j = k - 1;
          if (!knn_ahead(s, idx, list_s[j * KNN_TQ + tid],
                         list_i[j * KNN_TQ + tid]))
            continue;
          while (j > 0) {
            const float ps = list_s[(j - 1) * KNN_TQ + tid];
            const int pi = list_i[(j - 1) * KNN_TQ + tid];
            if (!knn_ahead(s, idx, ps, pi)) break;
            list_s[j * KNN_TQ + tid] = ps;
            list_i[j * KNN_TQ + tid] = pi;
            --j;
          }
          list_s[j * KNN_TQ + tid] = s;
          list_i[j * KNN_TQ + tid] = idx;
        }
      }
      __syncthreads();
      thr_s = list_s[(k - 1) * KNN_TQ + ql];
      thr_i = list_i[(k - 1) * KNN_TQ + ql];
    }
  }

  __syncthreads();
  for (int e = tid; e < k * KNN_TQ; e += 256) {
    const int q = e & (KNN_TQ - 1);
    const int j = e >> 7;
    if (q0 + q < n_q) {
      const long o = ((q0 + q) * splits + split) * k + j;
      part_s[o] = list_s[e];
      part_i[o] = list_i[e];
    }
  }
}

// One workgroup per query.  LDS: the query's splits*k pairs.  Every list is
// sorted and (+inf, -1) slots come last in it, so a live element's rank is
// its position plus the count of elements ahead of it in every other list
// (a binary search each).  Ranks of live elements are distinct.
extern "C" __global__ __launch_bounds__(128) void knn_merge_k(
    const float* __restrict__ part_s, const int* __restrict__ part_i,
    const float* __restrict__ qsq, int k, int splits,
    float* __restrict__ out_d2, int* __restrict__ out_idx) {
  extern __shared__ __attribute__((aligned(16))) float knn_lds[];
  const int E = splits * k;
  float* es = knn_lds;
  int* ei = (int*)(knn_lds + E);
  const long q = blockIdx.x;
  const int tid = threadIdx.x;
  for (int e = tid; e < E; e += 128) {
    es[e] = part_s[q * E + e];
    ei[e] = part_i[q * E + e];
  }
  for (int j = tid; j < k; j += 128) {
    out_d2[q * k + j] = __builtin_inff();
    out_idx[q * k + j] = -1;
  }
  __syncthreads();
  const float qq = qsq[q];
  for (int e = tid; e < E; e += 128) {
    const int idx = ei[e];
    if (idx < 0) continue;
    const float s = es[e];
    const int sp = e / k;
    int rank = e - sp * k;
    for (int o = 0; o < splits && rank < k; ++o) {
      if (o == sp) continue;
      int lo = 0, hi = k;   // first position of list o that is not ahead
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int mi = ei[o * k + mid];
        if (mi >= 0 && knn_ahead(es[o * k + mid], mi, s, idx)) lo = mid + 1;
        else hi = mid;
      }
      rank += lo;
    }
    if (rank < k) {
      out_d2[q * k + rank] = s + qq;
      out_idx[q * k + rank] = idx;
    }
  }
}

static inline size_t knn_partial_lds_bytes(int k) {
  return sizeof(float) * ((size_t)KNN_TN * KNN_LD + (size_t)KNN_TQ * KNN_LD +
                          KNN_TN + KNN_TN + KNN_TQ + 2 * (size_t)k * KNN_TQ);
}

// splits == 0: the workgroups run in rounds of `slots` = CUs x workgroups per
// CU (three by registers, fewer when k's lists fill the LDS); pick the split
// count whose last round is fullest, a larger count only when it gains two
// points of that share.  Each split stays at least eight index tiles long so
// the first tiles' selection rounds remain a small part of it.
extern "C" int knn_choose_splits(long n_q, long n, int k, int splits) {
  if (splits > 0) return splits;
  const long n_tiles = (n + KNN_TN - 1) / KNN_TN;
  const long q_tiles = (n_q + KNN_TQ - 1) / KNN_TQ;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                            dev) != hipSuccess || cus < 1)
    cus = 256;
  long per_cu = (long)(160 * 1024 / knn_partial_lds_bytes(k));
  if (per_cu > 3) per_cu = 3;
  if (per_cu < 1) per_cu = 1;
  const long slots = cus * per_cu;
  long s_max = n_tiles / 8;
  if (s_max > KNN_MAX_SPLITS) s_max = KNN_MAX_SPLITS;
  int best = 1;
  double best_fill = 0.0;
  for (long s = 1; s <= s_max; ++s) {
    const long blocks = q_tiles * s;
    const long rounds = (blocks + slots - 1) / slots;
    const double fill = (double)blocks / (double)(rounds * slots);
    if (fill > best_fill + 0.02) {
      best_fill = fill;
      best = (int)s;
    }
  }
  return best;
}

// part_s / part_i: n_q * splits * k scratch.  label_ids / allow_bits may both
// be null.  Returns a hipError_t as int.
extern "C" int launch_knn_topk(const float* Q, const float* X,
                               const float* xsq, const float* qsq,
                               const int* label_ids,
                               const unsigned* allow_bits, long n_q, long n,
                               int d, int k, int W, int splits, float* part_s,
                               int* part_i, float* out_d2, int* out_idx,
                               hipStream_t stream) {
  const long n_tiles = (n + KNN_TN - 1) / KNN_TN;
  long tps = (n_tiles + splits - 1) / splits;
  if (tps < 1) tps = 1;
  const long q_tiles = (n_q + KNN_TQ - 1) / KNN_TQ;
  const size_t lds = knn_partial_lds_bytes(k);
  hipError_t err = hipFuncSetAttribute(
      (const void*)knn_partial_topk_k,
      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(knn_partial_topk_k, dim3((unsigned)(q_tiles * splits)),
                     dim3(256), lds, stream, Q, X, xsq, label_ids, allow_bits,
                     n_q, (int)n, d, k, W, splits, (int)tps, part_s, part_i);
  hipLaunchKernelGGL(knn_merge_k, dim3((unsigned)n_q), dim3(128),
                     sizeof(float) * 2 * (size_t)splits * k, stream, part_s,
                     part_i, qsq, k, splits, out_d2, out_idx);
  return (int)hipGetLastError();
}
