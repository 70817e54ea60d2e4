// Alternating least squares for MI355X (gfx950): one half step, i.e. for every
// row u of a CSR matrix the normal equations A_u x_u = b_u against fixed
// factors Y, formed and solved inside one kernel.  No per-entry k x k
// temporaries exist anywhere; no float atomics are used, so the same inputs
// give the same bits on every run.
//
//   explicit  A_u = sum_e y_e y_e^T + reg I              b_u = sum_e r_e y_e
//   implicit  A_u = Y^T Y + sum_e a|r_e| y_e y_e^T + reg I
//             b_u = sum_{e: r_e > 0} (1 + a|r_e|) y_e    (Hu, Koren, Volinsky)
//
// Split of work
//   als_solve_rows_k<K>   a wavefront owns a row.  K is the rank padded to the
//       MFMA tile width (32 or 64); a block holds 4 (K = 32) or 3 (K = 64)
//       independent waves and never meets at a block barrier, so rows of very
//       different degree share a block without waiting for each other.  The
//       wave walks its entries in tiles of 32: lanes 0..31 read (col, val) and
//       turn val into the two weights (w for A, bw for b), then all 64 lanes
//       gather the 32 factor rows into an LDS tile (zero beyond the rank and
//       beyond the row's end).  The rank-32 update A += (w . Y_t)^T Y_t is
//       16 v_mfma_f32_32x32x2_f32 per 32 x 32 accumulator tile, two entries an
//       instruction; K = 64 keeps the three tiles (0,0), (1,0), (1,1) of the
//       lower triangle, 48 accumulator registers.  b is one fmaf chain per
//       lane over the tile's entries in CSR order.  After the last tile the
//       accumulators go to LDS (over the gather tile, which is dead by then),
//       Y^T Y and reg join the lower triangle, padded diagonal entries are set
//       to 1, and the wave factorises in place: left-looking Cholesky, lane i
//       owning row i (a column costs one wave-level sync), then the forward
//       and backward substitutions with the right-hand side in one register a
//       lane and __shfl for the pivot element.  Division and square root are
//       the correctly rounded ones, so the result obeys the textbook backward
//       error bound of Cholesky plus substitution.
//   als_solve_heavy_k<K>  access logs are power-law: rows whose degree exceeds
//       the heavy threshold (ALS_HEAVY_DEGREE, or the caller's value) are
//       skipped above and taken by a whole block each.  The block's waves
//       split the row's tiles into contiguous ranges that depend on the degree
//       alone, put their accumulators into their own LDS regions, and after
//       one barrier the regions are summed in wave order; wave 0 solves.  A
//       row's bits therefore depend on which side of the threshold it is, and
//       on nothing else.
//   als_gram_k<K> + als_gram_reduce_k  G = Y^T Y for the implicit mode.  Blocks
//       own contiguous chunks of rows of Y and run the same tile loop (no
//       gather, w = 1); block partials go to a scratch buffer and one thread
//       per entry of G sums them in block order in float64.
//   als_score_pairs_k     one thread per (user, resource) pair: the fmaf chain
//       of the two factor rows and the tenant's standardisation.
//
// LDS budget per wave (floats): the A region K (K + 1) (stride K + 1 keeps
// column walks off a single bank), whose first 32 (K + 1) floats double as the
// gather tile, K for b and 3 x 32 for w, bw and the column ids.  K = 64:
// 4160 + 64 + 96 = 4320 floats = 17280 B a wave, 51840 B a block of 3 waves,
// three blocks in a CU's 160 KB.  K = 32: 1056 + 32 + 96 = 1184 floats =
// 4736 B a wave, 18944 B a block of 4.
//
// MFMA at small ranks: at rank 10 nine tenths of a 32 x 32 tile is padding and
// a VALU loop over the 55 distinct products of an entry would issue fewer
// cycles (one 64-lane fma an entry against half a 64-cycle MFMA).  The MFMA
// path is kept for every rank all the same: it is one code path with one
// rounding behaviour, the matrix pipe runs beside the VALU and the gather, and
// at small ranks a row's time is the latency of the gathered loads and the
// serial Cholesky, not the update.  This is reasoning from instruction
// counts, not a measurement; a 16x16x4 variant for k <= 16 is the next step if
// a profile says otherwise.
#include <hip/hip_runtime.h>

#define ALS_MAX_K 64
#define ALS_TILE 32             // CSR entries per gather tile
#define ALS_HEAVY_DEGREE 1024   // rows with more entries get a whole block
#define ALS_GRAM_ROWS 256       // rows of Y per als_gram_k block, at least
#define ALS_GRAM_MAX_BLOCKS 2048

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int K>
struct AlsCfg {
  static constexpr int NT = K / 32;               // tile rows: 1 or 2
  static constexpr int NACC = NT * (NT + 1) / 2;  // lower-triangle tiles
  static constexpr int LD = K + 1;
  static constexpr int WAVES = K == 32 ? 4 : 3;
  static constexpr int A_FLOATS = K * LD;
  // [A | b | w | bw | col]; A and b are contiguous so partials sum in one loop
  static constexpr int WAVE_FLOATS = A_FLOATS + K + 3 * ALS_TILE;
};

// LDS traffic between the lanes of one wave: the hardware serves a wave's LDS
// instructions in order, so only the compiler has to be kept from moving them.
__device__ __forceinline__ void als_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int K>
struct AlsWaveLds {
  float* A;     // K x (K + 1); rows 0..31 hold the gather tile while it lives
  float* b;     // K
  float* w;     // 32 weights of A
  float* bw;    // 32 weights of b
  int* ci;      // 32 column ids
  __device__ __forceinline__ AlsWaveLds(float* base) {
    A = base;
    b = A + AlsCfg<K>::A_FLOATS;
    w = b + K;
    bw = w + ALS_TILE;
    ci = (int*)(bw + ALS_TILE);
  }
};

// acc += sum over entries [e_lo, e_hi) of w_e y_e y_e^T (lower tiles), bacc +=
// sum of bw_e y_e[lane].  GATHER: entry e is CSR entry e, y_e = Y[col[e]];
// otherwise y_e = Y[e], w = 1 and b is not formed.
template <int K, bool GATHER>
__device__ __forceinline__ void als_accumulate(
    const int* __restrict__ col, const float* __restrict__ val,
    const float* __restrict__ Y, int k, long e_lo, long e_hi, float alpha,
    int implicit, const AlsWaveLds<K>& s, int lane,
    f32x16 (&acc)[AlsCfg<K>::NACC], float& bacc) {
  constexpr int LD = AlsCfg<K>::LD;
  const int c32 = lane & 31;
  const int h = lane >> 5;
  float* tile = s.A;
  for (long e0 = e_lo; e0 < e_hi; e0 += ALS_TILE) {
    const int cnt = e_hi - e0 < ALS_TILE ? (int)(e_hi - e0) : ALS_TILE;
    als_wave_sync();   // the last tile's readers are done
    if (lane < ALS_TILE) {
      int c = 0;
      float w = 0.f, bw = 0.f;
      if (lane < cnt) {
        if (GATHER) {
          c = col[e0 + lane];
          const float r = val[e0 + lane];
          if (implicit) {
            w = alpha * __builtin_fabsf(r);
            bw = r > 0.f ? 1.f + w : 0.f;
          } else {
            w = 1.f;
            bw = r;
          }
        } else {
          c = (int)(e0 + lane);
          w = 1.f;
        }
      }
      s.w[lane] = w;
      s.bw[lane] = bw;
      s.ci[lane] = c;
    }
    als_wave_sync();
#pragma unroll 8
    for (int idx = lane; idx < ALS_TILE * K; idx += 64) {
      const int e = idx / K, f = idx % K;
      float y = 0.f;
      if (e < cnt && f < k) y = Y[(long)s.ci[e] * k + f];
      tile[e * LD + f] = y;
    }
    als_wave_sync();
    const int steps = (cnt + 1) >> 1;   // an odd count's last partner is zero
    for (int st = 0; st < steps; ++st) {
      const int e = 2 * st + h;
      const float w = s.w[e];
      const float y0 = tile[e * LD + c32];
      const float a0 = w * y0;
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, y0, acc[0], 0, 0, 0);
      if constexpr (K == 64) {
        const float y1 = tile[e * LD + 32 + c32];
        const float a1 = w * y1;
        acc[AlsCfg<K>::NACC - 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(
            a1, y0, acc[AlsCfg<K>::NACC - 2], 0, 0, 0);
        acc[AlsCfg<K>::NACC - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(
            a1, y1, acc[AlsCfg<K>::NACC - 1], 0, 0, 0);
      }
    }
    if (GATHER && lane < K) {
#pragma unroll 4
      for (int e = 0; e < cnt; ++e)
        bacc = __builtin_fmaf(s.bw[e], tile[e * LD + lane], bacc);
    }
  }
}

// Accumulators and b into the wave's LDS region.  Register r of a lane is row
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31 of its tile; the
// upper right tile of K = 64 is never written and never read.
template <int K>
__device__ __forceinline__ void als_dump(const AlsWaveLds<K>& s, int lane,
                                         const f32x16 (&acc)[AlsCfg<K>::NACC],
                                         float bacc) {
  constexpr int LD = AlsCfg<K>::LD;
  const int c32 = lane & 31;
  const int h = lane >> 5;
  als_wave_sync();   // the gather tile under A is dead
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
    s.A[i * LD + c32] = acc[0][r];
    if constexpr (K == 64) {
      s.A[(32 + i) * LD + c32] = acc[AlsCfg<K>::NACC - 2][r];
      s.A[(32 + i) * LD + 32 + c32] = acc[AlsCfg<K>::NACC - 1][r];
    }
  }
  if (lane < K) s.b[lane] = bacc;
  als_wave_sync();
}

// One wave: A (lower triangle in LDS) += G + reg I, Cholesky, two triangular
// solves, x_row written.  Rows and columns k..K-1 are the identity; they do
// not couple with the live ones, so the loops stop at k.
template <int K>
__device__ __forceinline__ void als_finish(const AlsWaveLds<K>& s, int lane,
                                           const float* __restrict__ G, int k,
                                           float reg, float* __restrict__ x) {
  constexpr int LD = AlsCfg<K>::LD;
  float* A = s.A;
  for (int idx = lane; idx < K * K; idx += 64) {
    const int i = idx / K, j = idx % K;
    if (j > i) continue;
    float a;
    if (i < k) {
      a = A[i * LD + j];
      if (G != nullptr) a += G[i * k + j];
      if (i == j) a += reg;
    } else {
      a = i == j ? 1.f : 0.f;
    }
    A[i * LD + j] = a;
  }
  als_wave_sync();

  const bool live = lane < k;
  for (int j = 0; j < k; ++j) {
    float v = 0.f;
    if (live && lane >= j) {
      v = A[lane * LD + j];
#pragma unroll 4
      for (int p = 0; p < j; ++p)
        v = __builtin_fmaf(-A[lane * LD + p], A[j * LD + p], v);
    }
    const float d = __builtin_sqrtf(__shfl(v, j));
    if (lane == j)
      A[j * LD + j] = d;
    else if (live && lane > j)
      A[lane * LD + j] = v / d;
    als_wave_sync();
  }

  float t = live ? s.b[lane] : 0.f;
  for (int j = 0; j < k; ++j) {          // L z = b
    const float z = __shfl(t, j) / A[j * LD + j];
    if (lane == j)
      t = z;
    else if (live && lane > j)
      t = __builtin_fmaf(-A[lane * LD + j], z, t);
  }
  for (int j = k - 1; j >= 0; --j) {     // L^T x = z
    const float xj = __shfl(t, j) / A[j * LD + j];
    if (lane == j)
      t = xj;
    else if (lane < j)
      t = __builtin_fmaf(-A[j * LD + lane], xj, t);
  }
  if (live) x[lane] = t;
}

template <int K>
__device__ __forceinline__ void als_zero(f32x16 (&acc)[AlsCfg<K>::NACC]) {
#pragma unroll
  for (int t = 0; t < AlsCfg<K>::NACC; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
}

template <int K>
__global__ __launch_bounds__(AlsCfg<K>::WAVES * 64) void als_solve_rows_k(
    const long* __restrict__ indptr, const int* __restrict__ col,
    const float* __restrict__ val, const float* __restrict__ Y,
    const float* __restrict__ G, int n_rows, int k, float reg, float alpha,
    int implicit, long heavy, float* __restrict__ x) {
  __shared__ float lds[AlsCfg<K>::WAVES * AlsCfg<K>::WAVE_FLOATS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * AlsCfg<K>::WAVES + wave;
  if (row >= n_rows) return;
  const long e_lo = indptr[row], e_hi = indptr[row + 1];
  if (e_hi - e_lo > heavy) return;       // als_solve_heavy_k takes it
  if (e_hi <= e_lo) {
    if (lane < k) x[row * k + lane] = 0.f;
    return;
  }
  const AlsWaveLds<K> s(lds + wave * AlsCfg<K>::WAVE_FLOATS);
  f32x16 acc[AlsCfg<K>::NACC];
  float bacc = 0.f;
  als_zero<K>(acc);
  als_accumulate<K, true>(col, val, Y, k, e_lo, e_hi, alpha, implicit, s, lane,
                          acc, bacc);
  als_dump<K>(s, lane, acc, bacc);
  als_finish<K>(s, lane, G, k, reg, x + row * k);
}

// Sum the waves' [A | b] regions into wave 0's, in wave order.
template <int K>
__device__ __forceinline__ void als_combine(float* lds, int n) {
  for (int idx = threadIdx.x; idx < n; idx += AlsCfg<K>::WAVES * 64) {
    float v = lds[idx];
#pragma unroll
    for (int w = 1; w < AlsCfg<K>::WAVES; ++w)
      v += lds[w * AlsCfg<K>::WAVE_FLOATS + idx];
    lds[idx] = v;
  }
}

// The contiguous share of [lo, hi) that `wave` takes, in whole tiles.
template <int K>
__device__ __forceinline__ void als_share(long lo, long hi, int wave,
                                          long& w_lo, long& w_hi) {
  const long tiles = (hi - lo + ALS_TILE - 1) / ALS_TILE;
  const long per = (tiles + AlsCfg<K>::WAVES - 1) / AlsCfg<K>::WAVES;
  w_lo = lo + wave * per * ALS_TILE;
  w_hi = w_lo + per * ALS_TILE;
  if (w_lo > hi) w_lo = hi;
  if (w_hi > hi) w_hi = hi;
}

template <int K>
__global__ __launch_bounds__(AlsCfg<K>::WAVES * 64) void als_solve_heavy_k(
    const long* __restrict__ indptr, const int* __restrict__ col,
    const float* __restrict__ val, const float* __restrict__ Y,
    const float* __restrict__ G, const int* __restrict__ heavy_rows, int k,
    float reg, float alpha, int implicit, float* __restrict__ x) {
  __shared__ float lds[AlsCfg<K>::WAVES * AlsCfg<K>::WAVE_FLOATS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long row = heavy_rows[blockIdx.x];
  long lo, hi;
  als_share<K>(indptr[row], indptr[row + 1], wave, lo, hi);
  const AlsWaveLds<K> s(lds + wave * AlsCfg<K>::WAVE_FLOATS);
  f32x16 acc[AlsCfg<K>::NACC];
  float bacc = 0.f;
  als_zero<K>(acc);
  als_accumulate<K, true>(col, val, Y, k, lo, hi, alpha, implicit, s, lane,
                          acc, bacc);
  als_dump<K>(s, lane, acc, bacc);
  __syncthreads();
  als_combine<K>(lds, AlsCfg<K>::A_FLOATS + K);
  __syncthreads();
  if (wave == 0) als_finish<K>(s, lane, G, k, reg, x + row * k);
}

template <int K>
__global__ __launch_bounds__(AlsCfg<K>::WAVES * 64) void als_gram_k(
    const float* __restrict__ Y, long n, int k, long rows_per_block,
    float* __restrict__ partial) {
  __shared__ float lds[AlsCfg<K>::WAVES * AlsCfg<K>::WAVE_FLOATS];
  constexpr int LD = AlsCfg<K>::LD;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.x * rows_per_block;
  long r1 = r0 + rows_per_block;
  if (r1 > n) r1 = n;
  long lo, hi;
  als_share<K>(r0, r1 > r0 ? r1 : r0, wave, lo, hi);
  const AlsWaveLds<K> s(lds + wave * AlsCfg<K>::WAVE_FLOATS);
  f32x16 acc[AlsCfg<K>::NACC];
  float bacc = 0.f;
  als_zero<K>(acc);
  als_accumulate<K, false>(nullptr, nullptr, Y, k, lo, hi, 0.f, 0, s, lane,
                           acc, bacc);
  als_dump<K>(s, lane, acc, bacc);
  __syncthreads();
  float* out = partial + (long)blockIdx.x * K * K;
  for (int idx = threadIdx.x; idx < K * K; idx += AlsCfg<K>::WAVES * 64) {
    const int i = idx / K, j = idx % K;
    if (j > i) continue;
    float v = lds[i * LD + j];
#pragma unroll
    for (int w = 1; w < AlsCfg<K>::WAVES; ++w)
      v += lds[w * AlsCfg<K>::WAVE_FLOATS + i * LD + j];
    out[idx] = v;
  }
}

// G[i][j] = G[j][i] = sum over blocks, in block order, in float64.
extern "C" __global__ __launch_bounds__(256) void als_gram_reduce_k(
    const float* __restrict__ partial, int blocks, int K, int k,
    float* __restrict__ G) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= k * k) return;
  const int i = idx / k, j = idx % k;
  if (j > i) return;
  double v = 0.0;
  for (int b = 0; b < blocks; ++b)
    v += (double)partial[(long)b * K * K + i * K + j];
  G[i * k + j] = (float)v;
  G[j * k + i] = (float)v;
}

// out[p] = (-(U[u_off[t] + user[p]] . V[v_off[t] + res[p]]) - mean[t]) / std[t]
// for tenant t = tenant[p]; NaN for an unknown tenant (t < 0) or an index
// outside the tenant's tables.  The dot is the fmaf chain in feature order.
extern "C" __global__ __launch_bounds__(256) void als_score_pairs_k(
    const float* __restrict__ U, const float* __restrict__ V,
    const int* __restrict__ user, const int* __restrict__ res,
    const int* __restrict__ tenant, const long* __restrict__ u_off,
    const long* __restrict__ v_off, const double* __restrict__ mean,
    const double* __restrict__ sd, int n_tenants, int k, long n,
    float* __restrict__ out) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int t = tenant[p];
  float r = __builtin_nanf("");
  if (t >= 0 && t < n_tenants) {
    const long u = user[p], v = res[p];
    const long nu = u_off[t + 1] - u_off[t], nv = v_off[t + 1] - v_off[t];
    if (u >= 0 && u < nu && v >= 0 && v < nv) {
      const float* a = U + (u_off[t] + u) * k;
      const float* b = V + (v_off[t] + v) * k;
      float dot = 0.f;
      for (int f = 0; f < k; ++f) dot = __builtin_fmaf(a[f], b[f], dot);
      r = (float)((-(double)dot - mean[t]) / sd[t]);
    }
  }
  out[p] = r;
}

extern "C" int als_heavy_degree() { return ALS_HEAVY_DEGREE; }

// Blocks of als_gram_k for n rows: a function of n alone, so G is repeatable.
extern "C" int als_gram_blocks(long n) {
  long b = (n + ALS_GRAM_ROWS - 1) / ALS_GRAM_ROWS;
  if (b < 1) b = 1;
  if (b > ALS_GRAM_MAX_BLOCKS) b = ALS_GRAM_MAX_BLOCKS;
  return (int)b;
}

// partial: als_gram_blocks(n) * K * K floats, K = 32 or 64 the padded rank.
extern "C" int launch_als_gram(const float* Y, long n, int k, float* partial,
                               float* G, hipStream_t stream) {
  const int blocks = als_gram_blocks(n);
  long rpb = (n + blocks - 1) / blocks;
  rpb = (rpb + ALS_TILE - 1) / ALS_TILE * ALS_TILE;
  if (rpb < ALS_TILE) rpb = ALS_TILE;
  const int K = k <= 32 ? 32 : 64;
  if (K == 32)
    hipLaunchKernelGGL(als_gram_k<32>, dim3(blocks),
                       dim3(AlsCfg<32>::WAVES * 64), 0, stream, Y, n, k, rpb,
                       partial);
  else
    hipLaunchKernelGGL(als_gram_k<64>, dim3(blocks),
                       dim3(AlsCfg<64>::WAVES * 64), 0, stream, Y, n, k, rpb,
                       partial);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(als_gram_reduce_k, dim3((k * k + 255) / 256), dim3(256),
                     0, stream, partial, blocks, K, k, G);
  return (int)hipGetLastError();
}

extern "C" int launch_als_solve_rows(const long* indptr, const int* col,
                                     const float* val, const float* Y,
                                     const float* G, int n_rows, int k,
                                     float reg, float alpha, int implicit,
                                     long heavy, float* x, hipStream_t stream) {
  if (k <= 32) {
    const unsigned blocks = (unsigned)(((long)n_rows + AlsCfg<32>::WAVES - 1) /
                                       AlsCfg<32>::WAVES);
    hipLaunchKernelGGL(als_solve_rows_k<32>, dim3(blocks),
                       dim3(AlsCfg<32>::WAVES * 64), 0, stream, indptr, col,
                       val, Y, G, n_rows, k, reg, alpha, implicit, heavy, x);
  } else {
    const unsigned blocks = (unsigned)(((long)n_rows + AlsCfg<64>::WAVES - 1) /
                                       AlsCfg<64>::WAVES);
    hipLaunchKernelGGL(als_solve_rows_k<64>, dim3(blocks),
                       dim3(AlsCfg<64>::WAVES * 64), 0, stream, indptr, col,
                       val, Y, G, n_rows, k, reg, alpha, implicit, heavy, x);
  }
  return (int)hipGetLastError();
}

extern "C" int launch_als_solve_heavy(const long* indptr, const int* col,
                                      const float* val, const float* Y,
                                      const float* G, const int* heavy_rows,
                                      int n_heavy, int k, float reg,
                                      float alpha, int implicit, float* x,
                                      hipStream_t stream) {
  if (k <= 32)
    hipLaunchKernelGGL(als_solve_heavy_k<32>, dim3(n_heavy),
                       dim3(AlsCfg<32>::WAVES * 64), 0, stream, indptr, col,
                       val, Y, G, heavy_rows, k, reg, alpha, implicit, x);
  else
    hipLaunchKernelGGL(als_solve_heavy_k<64>, dim3(n_heavy),
                       dim3(AlsCfg<64>::WAVES * 64), 0, stream, indptr, col,
                       val, Y, G, heavy_rows, k, reg, alpha, implicit, x);
  return (int)hipGetLastError();
}

extern "C" int launch_als_score_pairs(const float* U, const float* V,
                                      const int* user, const int* res,
                                      const int* tenant, const long* u_off,
                                      const long* v_off, const double* mean,
                                      const double* sd, int n_tenants, int k,
                                      long n, float* out, hipStream_t stream) {
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(als_score_pairs_k, dim3((unsigned)blocks), dim3(256), 0,
                     stream, U, V, user, res, tenant, u_off, v_off, mean, sd,
                     n_tenants, k, n, out);
  return (int)hipGetLastError();
}
