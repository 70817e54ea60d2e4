// Sparse SAR (item-item co-occurrence recommender) for MI355X (gfx950): no
// (users, items) or (items, items) matrix is ever formed.
//
// All matrices are CSR with int64 indptr, int32 columns strictly increasing
// inside a row, float32 values.  B is the binarised user-item matrix (an
// entry per interaction), Bt its transpose, A the affinity, S the similarity.
//
//   sar_cooc_count_k / sar_cooc_fill_k  grid = (item row i, item tile t).  A
//       block zeroes T u32 LDS cells and, for every user u of row i of Bt,
//       adds 1 to the cells of u's items inside [t*T, t*T + T): waves take
//       users, lanes take items, the range ends come from two binary searches
//       in u's sorted row.  Integer LDS atomics: the counts do not depend on
//       any order.  A cell is kept iff count >= thr (thr >= 1).  The count
//       pass writes the number of kept cells per (row, tile); the caller's
//       exclusive scan of that row-major array is every block's output
//       offset; the fill pass recomputes the tile and compacts the kept cells
//       in ascending column order (ballot/popc prefix per 256-cell chunk),
//       writing column and similarity.  occ_i = c_ii is the length of row i
//       of Bt, so no diagonal is looked up, and a row with occ_i < thr keeps
//       nothing and is left before any work.
//   sar_recommend_topk_k  one block per requested user, looping over item
//       tiles of T f32 LDS cells.  Scatter: for the user's entries in
//       ascending item i, cell[j] = fmaf(a_ui, s_ij, cell[j]) over row i of S.
//       Wave w owns cells [w*T/4, (w+1)*T/4) and searches its own piece of the
//       row, so a cell is only ever touched by one wave; a row's columns are
//       distinct, so one wave instruction never hits a cell twice, and a
//       wave's LDS operations retire in order: no atomics, no barrier between
//       entries, and every cell's addends arrive in ascending i whatever T is.
//       Selection: cells become order-preserving u32 keys (0 = not a
//       candidate: removed, past the last item, or not above the running
//       list's k-th score); if more than k candidates remain the tile's k-th
//       key is found by bisecting the 32 key bits with block-wide counts, and
//       ties at that key are cut by bisecting the cell index, so exactly k
//       cells win.  Winners join the running sorted list in LDS and one rank
//       sort under (score descending, item ascending) over at most 2k entries
//       keeps the best k.  Nothing depends on arrival order.
//   sar_score_pairs_k  thread per (user, item) pair: the same fmaf chain from
//       0.0f over the user's entries in ascending j with S[i, j] found by
//       binary search in row i (S is symmetric), hence the same bits as the
//       score sar_recommend_topk_k reports for that pair.
//
// Every index that addresses LDS or picks a row is range-checked here again,
// although the host validates the structures before any launch.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define SAR_MAX_K 128
#define SAR_MAX_TILE 16384

// first position in col[lo, hi) whose value is >= key
__device__ __forceinline__ long sar_lower_bound(const int* __restrict__ col,
                                                long lo, long hi, long key) {
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if ((long)col[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Block-wide sum of v over 256 threads, one barrier.  red holds two slots of
// four words used alternately: a slot is rewritten two calls later, after a
// barrier that every thread reaches only once it has read the slot.
__device__ __forceinline__ int sar_block_sum(int v, volatile int* red,
                                             int& parity) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  volatile int* slot = red + parity * 4;
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
  __syncthreads();
  const int s = slot[0] + slot[1] + slot[2] + slot[3];
  parity ^= 1;
  return s;
}

// cells[0, T) <- co-occurrence counts of item i with items [c0, c0 + T)
__device__ __forceinline__ void sar_cooc_tile(
    unsigned* cells, const long* __restrict__ bt_indptr,
    const int* __restrict__ bt_col, const long* __restrict__ b_indptr,
    const int* __restrict__ b_col, int n_users, int i, long c0, int T) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  for (int c = tid; c < T; c += 256) cells[c] = 0u;
  __syncthreads();
  const long r0 = bt_indptr[i], r1 = bt_indptr[i + 1];
  for (long p = r0 + wave; p < r1; p += 4) {
    const int u = bt_col[p];
    if (u < 0 || u >= n_users) continue;
    const long u0 = b_indptr[u], u1 = b_indptr[u + 1];
    const long lo = sar_lower_bound(b_col, u0, u1, c0);
    const long hi = sar_lower_bound(b_col, lo, u1, c0 + T);
    for (long q = lo + lane; q < hi; q += 64) {
      const long cell = (long)b_col[q] - c0;
      if (cell >= 0 && cell < T) atomicAdd(&cells[cell], 1u);
    }
  }
  __syncthreads();
}

// LDS (dynamic, words): [cells T | red 8]
extern "C" __global__ __launch_bounds__(256) void sar_cooc_count_k(
    const long* __restrict__ bt_indptr, const int* __restrict__ bt_col,
    const long* __restrict__ b_indptr, const int* __restrict__ b_col,
    int n_users, int n_items, int T, unsigned thr, int* __restrict__ counts) {
  extern __shared__ unsigned sar_cooc_lds[];
  unsigned* cells = sar_cooc_lds;
  volatile int* red = (volatile int*)(cells + T);
  const int tid = threadIdx.x;
  const int i = blockIdx.x;
  const long slot = (long)i * gridDim.y + blockIdx.y;
  const long c0 = (long)blockIdx.y * T;
  const long occ_i = bt_indptr[i + 1] - bt_indptr[i];
  if (occ_i < (long)thr) {          // c_ij <= occ_i: nothing can be kept
    if (tid == 0) counts[slot] = 0;
    return;
  }
  sar_cooc_tile(cells, bt_indptr, bt_col, b_indptr, b_col, n_users, i, c0, T);
  int n = 0;
  for (int c = tid; c < T; c += 256) n += cells[c] >= thr;
  int parity = 0;
  n = sar_block_sum(n, red, parity);
  if (tid == 0) counts[slot] = n;
}

// sim: 0 cooccurrence, 1 jaccard, 2 lift
extern "C" __global__ __launch_bounds__(256) void sar_cooc_fill_k(
    const long* __restrict__ bt_indptr, const int* __restrict__ bt_col,
    const long* __restrict__ b_indptr, const int* __restrict__ b_col,
    int n_users, int n_items, int T, unsigned thr, int sim,
    const long* __restrict__ offsets, long nnz, int* __restrict__ out_col,
    float* __restrict__ out_val) {
  extern __shared__ unsigned sar_cooc_lds[];
  unsigned* cells = sar_cooc_lds;
  volatile int* wcnt = (volatile int*)(cells + T);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int i = blockIdx.x;
  const long slot = (long)i * gridDim.y + blockIdx.y;
  const long c0 = (long)blockIdx.y * T;
  const long occ_i = bt_indptr[i + 1] - bt_indptr[i];
  if (occ_i < (long)thr) return;
  sar_cooc_tile(cells, bt_indptr, bt_col, b_indptr, b_col, n_users, i, c0, T);
  long out = offsets[slot];
  for (int base = 0; base < T; base += 256) {
    const int c = base + tid;
    const unsigned cnt = c < T ? cells[c] : 0u;
    const bool keep = cnt >= thr && c0 + c < n_items;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wcnt[(base >> 8 & 1) * 4 + wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int v = wcnt[(base >> 8 & 1) * 4 + w];
      if (w < wave) before += v;
      total += v;
    }
    if (keep) {
      const long j = c0 + c;
      const long pos = out + before + __popcll(m & ((1ull << lane) - 1ull));
      if (pos >= 0 && pos < nnz) {
        const long occ_j = bt_indptr[j + 1] - bt_indptr[j];
        float v = (float)cnt;
        if (sim == 1)
          v = (float)cnt / (float)(occ_i + occ_j - (long)cnt);
        else if (sim == 2)
          v = (float)cnt / ((float)occ_i * (float)occ_j);
        out_col[pos] = (int)j;
        out_val[pos] = v;
      }
    }
    out += total;
  }
}

// order-preserving key of a score: a > b  <=>  key(a) > key(b); never 0 for
// a score above -inf
__device__ __forceinline__ unsigned sar_key(float s) {
  const unsigned b = __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sar_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ bool sar_ahead(float s, int i, float ts, int ti) {
  return s > ts || (s == ts && i < ti);
}

// LDS (dynamic, words): [cells T | comb_s 2k | comb_i 2k | red 8 | nwin 1]
extern "C" __global__ __launch_bounds__(256) void sar_recommend_topk_k(
    const long* __restrict__ a_indptr, const int* __restrict__ a_col,
    const float* __restrict__ a_val, const long* __restrict__ s_indptr,
    const int* __restrict__ s_col, const float* __restrict__ s_val,
    const int* __restrict__ users, int n_users, int n_items, int T, int k,
    int remove_seen, float* __restrict__ out_s, int* __restrict__ out_i) {
  extern __shared__ unsigned sar_rec_lds[];
  unsigned* cells = sar_rec_lds;
  volatile unsigned* vcells = cells;
  float* comb_s = (float*)(cells + T);
  int* comb_i = (int*)(comb_s + 2 * k);
  volatile int* red = (volatile int*)(comb_i + 2 * k);
  int* nwin = (int*)(red + 8);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const long r = blockIdx.x;
  const int u = users != nullptr ? users[r] : (int)r;
  const float ninf = -__builtin_inff();
  if (u < 0 || u >= n_users) {
    if (tid < k) { out_s[r * k + tid] = ninf; out_i[r * k + tid] = -1; }
    return;
  }
  const long e0 = a_indptr[u], e1 = a_indptr[u + 1];
  const int sub = T >> 2;                   // cells owned by one wave
  const int own_lo = wave * sub, own_hi = own_lo + sub;
  int L = 0;                                // entries in the running list
  int parity = 0;

  for (long c0 = 0; c0 < n_items; c0 += T) {
    for (int c = tid; c < T; c += 256) cells[c] = 0u;   // +0.0f
    if (tid == 0) *nwin = 0;
    __syncthreads();

    for (long e = e0; e < e1; ++e) {
      const int i = a_col[e];
      if (i < 0 || i >= n_items) continue;
      const float a = a_val[e];
      const long s0 = s_indptr[i], s1 = s_indptr[i + 1];
      const long lo = sar_lower_bound(s_col, s0, s1, c0 + own_lo);
      const long hi = sar_lower_bound(s_col, lo, s1, c0 + own_hi);
      for (long q = lo + lane; q < hi; q += 64) {
        const long cell = (long)s_col[q] - c0;
        if (cell >= own_lo && cell < own_hi)
          vcells[cell] = __float_as_uint(
              fmaf(a, s_val[q], __uint_as_float(vcells[cell])));
      }
    }
    __syncthreads();
    if (remove_seen) {
      for (long e = e0 + lane; e < e1; e += 64) {
        const long cell = (long)a_col[e] - c0;
        if (a_val[e] > 0.f && cell >= own_lo && cell < own_hi)
          cells[cell] = __float_as_uint(ninf);
      }
      __syncthreads();
    }

    // cells -> keys; candidates are above the list's k-th score (a tie with
    // it loses: every item here has a larger index than any in the list)
    const float thr_s = L == k ? comb_s[k - 1] : ninf;
    int n = 0;
    for (int c = tid; c < T; c += 256) {
      const float s = __uint_as_float(cells[c]) + 0.0f;
      const bool cand = c0 + c < n_items && s > thr_s;
      cells[c] = cand ? sar_key(s) : 0u;
      n += cand;
    }
    const int ncand = sar_block_sum(n, red, parity);
    if (ncand == 0) continue;

    // winners: key > vh, or key == vh && c <= cmax.  With at most k
    // candidates every one of them (key != 0) wins.
    unsigned vh = 0u;
    int cmax = -1;
    if (ncand > k) {
      for (int bit = 31; bit >= 0; --bit) {
        const unsigned trial = vh | (1u << bit);
        n = 0;
        for (int c = tid; c < T; c += 256) n += cells[c] >= trial;
        if (sar_block_sum(n, red, parity) >= k) vh = trial;
      }
      // vh is the k-th largest key: fewer than k cells are above it
      n = 0;
      for (int c = tid; c < T; c += 256) {
        const unsigned key = cells[c];
        n += (key > vh) + ((key >= vh) << 16);
      }
      n = sar_block_sum(n, red, parity);
      const int need = k - (n & 0xffff);       // ties to take, >= 1
      cmax = T - 1;
      if ((n >> 16) > k) {                      // more ties than places
        int lo = 0, hi = T - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          n = 0;
          for (int c = tid; c <= mid; c += 256) n += cells[c] == vh;
          if (sar_block_sum(n, red, parity) >= need) hi = mid; else lo = mid + 1;
        }
        cmax = lo;
      }
    }

    for (int c = tid; c < T; c += 256) {
      const unsigned key = cells[c];
      if (key > vh || (key == vh && c <= cmax)) {
        const int slot = atomicAdd(nwin, 1);
        if (slot < k) {
          comb_s[L + slot] = sar_unkey(key);
          comb_i[L + slot] = (int)(c0 + c);
        }
      }
    }
    __syncthreads();
    int m = *nwin;
    if (m > k) m = k;
    const int tot = L + m;                     // <= 2k <= 256
    float ms = 0.f;
    int mi = 0, rank = 0;
    if (tid < tot) {
      ms = comb_s[tid];
      mi = comb_i[tid];
      for (int j = 0; j < tot; ++j)
        rank += sar_ahead(comb_s[j], comb_i[j], ms, mi);
    }
    __syncthreads();
    if (tid < tot && rank < 2 * k) { comb_s[rank] = ms; comb_i[rank] = mi; }
    L = tot < k ? tot : k;
    __syncthreads();
  }

  if (tid < k) {
    out_s[r * k + tid] = tid < L ? comb_s[tid] : ninf;
    out_i[r * k + tid] = tid < L ? comb_i[tid] : -1;
  }
}

extern "C" __global__ __launch_bounds__(256) void sar_score_pairs_k(
    const long* __restrict__ a_indptr, const int* __restrict__ a_col,
    const float* __restrict__ a_val, const long* __restrict__ s_indptr,
    const int* __restrict__ s_col, const float* __restrict__ s_val,
    const int* __restrict__ users, const int* __restrict__ items, long n_pairs,
    int n_users, int n_items, float* __restrict__ out) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pairs) return;
  const int u = users[p], i = items[p];
  if (u < 0 || u >= n_users || i < 0 || i >= n_items) { out[p] = 0.f; return; }
  const long r1 = s_indptr[i + 1];
  long lo = s_indptr[i];
  float acc = 0.0f;
  for (long e = a_indptr[u]; e < a_indptr[u + 1] && lo < r1; ++e) {
    const int j = a_col[e];
    lo = sar_lower_bound(s_col, lo, r1, j);
    if (lo < r1 && s_col[lo] == j) acc = fmaf(a_val[e], s_val[lo], acc);
  }
  out[p] = acc + 0.0f;
}

// ---------------------------------------------------------------- launchers
// The tile a launcher picks when the caller passes 0: every item in one tile
// when that fits (the fastest of a sweep at 5000 items for both tiled
// kernels, docs/kernels.md), else the cap.  which: 0 co-occurrence,
// 1 recommend.
extern "C" int sar_default_tile(long n_items, int which) {
  (void)which;
  const long cap = 8192;
  long t = (n_items + 63) / 64 * 64;
  if (t < 64) t = 64;
  return (int)(t < cap ? t : cap);
}

extern "C" int launch_sar_cooc_count(const long* bt_indptr, const int* bt_col,
                                     const long* b_indptr, const int* b_col,
                                     int n_users, int n_items, int T,
                                     unsigned thr, int* counts,
                                     hipStream_t stream) {
  const long n_tiles = ((long)n_items + T - 1) / T;
  const size_t lds = sizeof(unsigned) * ((size_t)T + 8);
  hipError_t err = hipFuncSetAttribute(
      (const void*)sar_cooc_count_k,
      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(sar_cooc_count_k,
                     dim3((unsigned)n_items, (unsigned)n_tiles), dim3(256),
                     lds, stream, bt_indptr, bt_col, b_indptr, b_col, n_users,
                     n_items, T, thr, counts);
  return (int)hipGetLastError();
}

extern "C" int launch_sar_cooc_fill(const long* bt_indptr, const int* bt_col,
                                    const long* b_indptr, const int* b_col,
                                    int n_users, int n_items, int T,
                                    unsigned thr, int sim, const long* offsets,
                                    long nnz, int* out_col, float* out_val,
                                    hipStream_t stream) {
  const long n_tiles = ((long)n_items + T - 1) / T;
  const size_t lds = sizeof(unsigned) * ((size_t)T + 8);
  hipError_t err = hipFuncSetAttribute(
      (const void*)sar_cooc_fill_k,
      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(sar_cooc_fill_k,
                     dim3((unsigned)n_items, (unsigned)n_tiles), dim3(256),
                     lds, stream, bt_indptr, bt_col, b_indptr, b_col, n_users,
                     n_items, T, thr, sim, offsets, nnz, out_col, out_val);
  return (int)hipGetLastError();
}

extern "C" int launch_sar_recommend(const long* a_indptr, const int* a_col,
                                    const float* a_val, const long* s_indptr,
                                    const int* s_col, const float* s_val,
                                    const int* users, long n_rows, int n_users,
                                    int n_items, int T, int k, int remove_seen,
                                    float* out_s, int* out_i,
                                    hipStream_t stream) {
  const size_t lds = sizeof(unsigned) * ((size_t)T + 4 * (size_t)k + 9);
  hipError_t err = hipFuncSetAttribute(
      (const void*)sar_recommend_topk_k,
      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(sar_recommend_topk_k, dim3((unsigned)n_rows), dim3(256),
                     lds, stream, a_indptr, a_col, a_val, s_indptr, s_col,
                     s_val, users, n_users, n_items, T, k, remove_seen, out_s,
                     out_i);
  return (int)hipGetLastError();
}

extern "C" int launch_sar_score_pairs(const long* a_indptr, const int* a_col,
                                      const float* a_val, const long* s_indptr,
                                      const int* s_col, const float* s_val,
                                      const int* users, const int* items,
                                      long n_pairs, int n_users, int n_items,
                                      float* out, hipStream_t stream) {
  const long blocks = (n_pairs + 255) / 256;
  hipLaunchKernelGGL(sar_score_pairs_k, dim3((unsigned)blocks), dim3(256), 0,
                     stream, a_indptr, a_col, a_val, s_indptr, s_col, s_val,
                     users, items, n_pairs, n_users, n_items, out);
  return (int)hipGetLastError();
}
