// LIME's local lasso surrogates, every fit of a chunk in one launch.
//
// One block of 8 wavefronts per explained row r.  The row's n on/off states
// (bit rows, cpu_ref.pack_states), its kernel weights and its Gram matrix are
// shared by the row's C classes, so the block
//   1. sums the kernel weights sqrt(exp(-(d / width)^2)), d = sqrt(#off / m),
//      in a fixed order (strided partials, then a tree), to normalise them;
//   2. forms the augmented Gram A' diag(w) A of A = [S | 1 | Y], m + 1 + C
//      columns, with v_mfma_f64_16x16x4f64: the samples pass through LDS 64 at
//      a time as packed words, each lane unpacks its bit, the A operand is
//      w_i * a_ic and the B operand a_ic'.  The upper-triangle 16 x 16 tiles
//      are dealt round robin to the waves, LF_ACC accumulators a wave, and
//      mirrored when stored.  S'WS goes to the Gram store G (m x m), the
//      1 + C other rows (weighted means, S'Wy, ym, y'Wy) to `aux` in LDS.
//      Integer per-column on-counts are taken from the same staged words;
//   3. standardises in place: cov = G - xm xm', xs = sqrt(diag cov),
//      G <- cov / (xs xs').  A column whose count is 0 or n is constant: it
//      is left out of the descent and its coefficient is exactly 0;
//   4. runs the cyclic coordinate descent of explainers/regression.py::
//      lasso_regression in covariance form, one wavefront per class:
//      q = c - G beta lives in registers, lane l owning coordinates l,
//      l + 64, ...; a step reads rho = q_j + G_jj beta_j from its owner lane,
//      soft-thresholds, and subtracts G[:, j] * delta.  No reduction and no
//      block barrier inside a sweep.  Same order, same bnew != bj test, same
//      max |delta| < tol stop after a full sweep and the same max_iter, so
//      the iterates are the host's in exact arithmetic.
//
// Two instantiations: m <= 128 keeps G in LDS (128 KiB); 128 < m <= 512 keeps
// it in a per-row global scratch the launcher hands in, which stays in L2 and
// whose row j the descent reads coalesced, one row ahead.
// Everything is float64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LIME_FIT_MAX_FEATURES 512
#define LIME_FIT_MAX_OUTPUTS 8
#define LF_LDS_FEATURES 128   // largest m whose Gram stays in LDS
#define LF_THREADS 512
#define LF_WAVES (LF_THREADS / 64)
#define LF_CHUNK 64           // samples staged per barrier (16 MFMA K steps)
#define LF_ACC 8              // 16 x 16 tiles a wave accumulates per pass;
                              // 12 and 16 spill vector registers

typedef double lf_d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double lf_bcast(double v, int src_lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, src_lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src_lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ double lf_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sqrt(exp(-(d / width)^2)) with d = sqrt(off / m)   (LIMEBase._weights)
__device__ __forceinline__ double lf_weight(int off, int m, double width) {
  const double d = sqrt((double)off) / sqrt((double)m);
  const double z = d / width;
  return sqrt(exp(-(z * z)));
}

__device__ __forceinline__ int lf_on_bits(const unsigned* row, int W,
                                          unsigned last_mask) {
  int on = 0;
  for (int k = 0; k < W - 1; ++k) on += __popc(row[k]);
  return on + __popc(row[W - 1] & last_mask);
}

// value of column c of A = [S | 1 | Y] at staged sample sl
__device__ __forceinline__ double lf_col(const unsigned* s_words,
                                         const double* s_y, int sl, int c,
                                         int m, int W, int C) {
  if (c < m) return (double)((s_words[sl * W + (c >> 5)] >> (c & 31)) & 1u);
  if (c == m) return 1.0;
  const int k = c - m - 1;
  return k < C ? s_y[sl * C + k] : 0.0;
}

template <int KPER>
__device__ __forceinline__ double lf_pick(const double (&v)[KPER], int slot) {
  double r = v[0];
#pragma unroll
  for (int k = 1; k < KPER; ++k) r = (k == slot) ? v[k] : r;
  return r;
}

// MAXM / 64 coordinates per lane; GLOBAL_GRAM: G lives in `gram_scratch`.
template <int MAXM, bool GLOBAL_GRAM>
__global__ __launch_bounds__(LF_THREADS) void lime_fit_k(
    const unsigned* __restrict__ states, const double* __restrict__ scores,
    int n, int m, int C, double width, double alpha, int max_iter, double tol,
    double* __restrict__ gram_scratch, double* __restrict__ coef,
    double* __restrict__ intercept, double* __restrict__ r2,
    int* __restrict__ n_sweeps) {
  constexpr int KPER = MAXM / 64;
  extern __shared__ double lf_lds[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);   // wave-uniform
  const long r = blockIdx.x;
  const int W = (m + 31) >> 5;
  const int P = m + 1 + C;
  const int T = (P + 15) >> 4;
  const unsigned last_mask = (m & 31) ? ((1u << (m & 31)) - 1u) : 0xffffffffu;

  // LDS carve-up (the launcher sizes it with lf_lds_bytes)
  double* G = GLOBAL_GRAM ? gram_scratch + r * (long)m * m : lf_lds;
  double* aux = lf_lds + (GLOBAL_GRAM ? 0 : (long)m * m);   // (1 + C, P)
  double* s_xm = aux + (1 + C) * P;                         // m
  double* s_xs = s_xm + m;                                  // m, 0 = constant
  double* s_y = s_xs + m;               // LF_CHUNK * C, also the sum tree
  double* s_w = s_y + LF_THREADS;                           // LF_CHUNK
  unsigned* s_words = (unsigned*)(s_w + LF_CHUNK);          // LF_CHUNK * W

  const unsigned* st_r = states + r * (long)n * W;
  const double* sc_r = scores + r * (long)n * C;

  // ---- 1. weight sum, fixed order
  {
    double part = 0.0;
    for (int s = t; s < n; s += LF_THREADS)
      part += lf_weight(m - lf_on_bits(st_r + (long)s * W, W, last_mask), m,
                        width);
    s_y[t] = part;
    __syncthreads();
    for (int h = LF_THREADS / 2; h >= 1; h >>= 1) {
      if (t < h) s_y[t] += s_y[t + h];
      __syncthreads();
    }
  }
  const double wsum = s_y[0];
  __syncthreads();

  // ---- 2. augmented Gram by f64 MFMA
  const int n_pairs = T * (T + 1) / 2;
  int count = 0;   // thread j < m: samples with column j on
  for (int p0 = 0; p0 < n_pairs; p0 += LF_WAVES * LF_ACC) {
    int ti[LF_ACC], tj[LF_ACC];
    lf_d4 acc[LF_ACC];
#pragma unroll
    for (int k = 0; k < LF_ACC; ++k) {
      int rem = p0 + k * LF_WAVES + wave, a = 0;
      if (rem >= n_pairs) { ti[k] = -1; tj[k] = -1; }
      else {
        while (rem >= T - a) { rem -= T - a; ++a; }
        ti[k] = a; tj[k] = a + rem;
      }
      acc[k] = (lf_d4){0.0, 0.0, 0.0, 0.0};
    }
    for (int s0 = 0; s0 < n; s0 += LF_CHUNK) {
      __syncthreads();
      for (int i = t; i < LF_CHUNK * W; i += LF_THREADS) {
        const int s = s0 + i / W;
        s_words[i] = s < n ? st_r[(long)s0 * W + i] : 0u;
      }
      for (int i = t; i < LF_CHUNK * C; i += LF_THREADS) {
        const int s = s0 + i / C;
        s_y[i] = s < n ? sc_r[(long)s0 * C + i] : 0.0;
      }
      __syncthreads();
      if (t < LF_CHUNK) {
        const int off = m - lf_on_bits(s_words + t * W, W, last_mask);
        s_w[t] = s0 + t < n ? lf_weight(off, m, width) / wsum : 0.0;
      }
      if (p0 == 0 && t < m) {
        const int lim = min(LF_CHUNK, n - s0);
        for (int s = 0; s < lim; ++s)
          count += (s_words[s * W + (t >> 5)] >> (t & 31)) & 1u;
      }
      __syncthreads();
      const int steps = (min(LF_CHUNK, n - s0) + 3) >> 2;
      for (int ks = 0; ks < steps; ++ks) {
        const int sl = ks * 4 + (lane >> 4);
        const double w = s_w[sl];
#pragma unroll
        for (int k = 0; k < LF_ACC; ++k) {
          if (ti[k] >= 0) {
            const double a = w * lf_col(s_words, s_y, sl,
                                        ti[k] * 16 + (lane & 15), m, W, C);
            const double b = lf_col(s_words, s_y, sl,
                                    tj[k] * 16 + (lane & 15), m, W, C);
            acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[k], 0, 0,
                                                          0);
          }
        }
      }
    }
    // lane l holds D[4 * v + l / 16][l % 16] in element v
#pragma unroll
    for (int k = 0; k < LF_ACC; ++k) {
      if (ti[k] < 0) continue;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int i = ti[k] * 16 + 4 * v + (lane >> 4);
        const int j = tj[k] * 16 + (lane & 15);
        if (i >= P || j >= P) continue;
        const double d = acc[k][v];
        const bool mirror = ti[k] != tj[k];   // then i < j
        if (i < m && j < m) {
          G[(long)i * m + j] = d;
          if (mirror) G[(long)j * m + i] = d;
        } else if (i >= m) {                  // row i - m of aux
          aux[(i - m) * P + j] = d;
          if (mirror) aux[(j - m) * P + i] = d;   // i >= m and i < j: j >= m
        } else {                              // i < m <= j: column i of aux
          aux[(j - m) * P + i] = d;
        }
      }
    }
  }
  __syncthreads();

  // ---- 3. standardise in place
  if (t < m) {
    const double xm = aux[t];
    const double var = G[(long)t * m + t] - xm * xm;
    s_xm[t] = xm;
    s_xs[t] = (count > 0 && count < n && var > 0.0) ? sqrt(var) : 0.0;
  }
  __syncthreads();
  for (long i = t; i < (long)m * m; i += LF_THREADS) {
    const int j = (int)(i / m), k = (int)(i - (long)j * m);
    const double sj = s_xs[j], sk = s_xs[k];
    G[i] = (sj > 0.0 && sk > 0.0)
               ? (G[i] - s_xm[j] * s_xm[k]) / (sj * sk) : 0.0;
  }
  __syncthreads();

  // ---- 4. covariance-form coordinate descent, one wavefront per class
  for (int c = wave; c < C; c += LF_WAVES) {
    const double* ay = aux + (1 + c) * P;     // column m + 1 + c against all
    const double ym = aux[m + 1 + c];
    const double var = ay[m + 1 + c] - ym * ym;
    double q[KPER], beta[KPER], cc[KPER], z[KPER];
#pragma unroll
    for (int k = 0; k < KPER; ++k) {
      const int j = lane + 64 * k;
      const double xs = j < m ? s_xs[j] : 0.0;
      cc[k] = xs > 0.0 ? (ay[j] - s_xm[j] * ym) / xs : 0.0;
      z[k] = xs > 0.0 ? G[(long)j * m + j] : 1.0;
      q[k] = cc[k];
      beta[k] = 0.0;
    }
    int sweeps = 0;
    for (; sweeps < max_iter;) {
      double max_delta = 0.0;
      double gn[KPER];
#pragma unroll
      for (int k = 0; k < KPER; ++k)
        gn[k] = lane + 64 * k < m ? G[lane + 64 * k] : 0.0;
      for (int j = 0; j < m; ++j) {
        double g[KPER];
        const long next = j + 1 < m ? (long)(j + 1) * m : 0;
#pragma unroll
        for (int k = 0; k < KPER; ++k) {
          g[k] = gn[k];
          gn[k] = lane + 64 * k < m ? G[next + lane + 64 * k] : 0.0;
        }
        if (!(s_xs[j] > 0.0)) continue;
        const int slot = j >> 6, owner = j & 63;
        const double bj = lf_bcast(lf_pick<KPER>(beta, slot), owner);
        const double zj = lf_bcast(lf_pick<KPER>(z, slot), owner);
        const double rho =
            lf_bcast(lf_pick<KPER>(q, slot), owner) + zj * bj;
        const double mag = fmax(fabs(rho) - alpha, 0.0);
        const double bnew =
            (rho > 0.0 ? mag : (rho < 0.0 ? -mag : 0.0 * mag)) / zj;
        if (bnew != bj) {
          const double delta = bnew - bj;
#pragma unroll
          for (int k = 0; k < KPER; ++k) {
            q[k] -= g[k] * delta;
            if (k == slot && lane == owner) beta[k] = bnew;
          }
          max_delta = fmax(max_delta, fabs(delta));
        }
      }
      ++sweeps;
      if (max_delta < tol) break;
    }
    double dot_xm = 0.0, dot_fit = 0.0;
    double* coef_rc = coef + (r * C + c) * (long)m;
#pragma unroll
    for (int k = 0; k < KPER; ++k) {
      const int j = lane + 64 * k;
      if (j < m) {
        const double xs = s_xs[j];
        const double cf = xs > 0.0 ? beta[k] / xs : 0.0;
        coef_rc[j] = cf;
        dot_xm += cf * s_xm[j];
        dot_fit += beta[k] * (cc[k] + q[k]);   // 2 b'c - b'Gb = b'(c + q)
      }
    }
    dot_xm = lf_wave_sum(dot_xm);
    dot_fit = lf_wave_sum(dot_fit);
    if (lane == 0) {
      intercept[r * C + c] = ym - dot_xm;
      r2[r * C + c] = 1.0 - (var - dot_fit) / fmax(var, 1e-12);
      n_sweeps[r * C + c] = sweeps;
    }
  }
}

static size_t lf_lds_bytes(int m, int C, bool global_gram) {
  const int W = (m + 31) / 32, P = m + 1 + C;
  size_t d = (size_t)(1 + C) * P + 2 * (size_t)m + LF_THREADS + LF_CHUNK;
  if (!global_gram) d += (size_t)m * m;
  return d * sizeof(double) + (size_t)LF_CHUNK * W * sizeof(unsigned);
}

extern "C" int lime_fit_max_features() { return LIME_FIT_MAX_FEATURES; }
extern "C" int lime_fit_max_outputs() { return LIME_FIT_MAX_OUTPUTS; }

// doubles of per-row Gram scratch the launch needs (0: the Gram fits in LDS)
extern "C" long lime_fit_scratch_doubles(int m) {
  return m > LF_LDS_FEATURES ? (long)m * m : 0;
}

extern "C" int launch_lime_fit(const int* states, const double* scores, int R,
                               int n, int m, int C, double width, double alpha,
                               int max_iter, double tol, double* gram_scratch,
                               double* coef, double* intercept, double* r2,
                               int* n_sweeps, hipStream_t stream) {
  if (R < 1 || n < 1 || m < 1 || m > LIME_FIT_MAX_FEATURES || C < 1 ||
      C > LIME_FIT_MAX_OUTPUTS || max_iter < 0 || !(width > 0.0) ||
      !(alpha >= 0.0))
    return -1;
  const bool global_gram = m > LF_LDS_FEATURES;
  if (global_gram && gram_scratch == nullptr) return -1;
  const size_t lds = lf_lds_bytes(m, C, global_gram);
  auto kern = global_gram ? lime_fit_k<LIME_FIT_MAX_FEATURES, true>
                          : lime_fit_k<LF_LDS_FEATURES, false>;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(
        (const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(R), dim3(LF_THREADS), lds, stream,
                     (const unsigned*)states, scores, n, m, C, width, alpha,
                     max_iter, tol, gram_scratch, coef, intercept, r2,
                     n_sweeps);
  return (int)hipGetLastError();
}
