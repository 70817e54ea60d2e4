// CDNA4 kernels for VW's -q: hashed sparse SGD and scoring over a COMPACT
// batch that stores each namespace (feature column) of an example once and
// generates the crossed features a x b in registers, the way VW enumerates
// them inside its learn loop.  Nothing of size |A|*|B| is ever stored.
//
// Batch: idx/val hold the raw per-column entries; ns_off (n_ex, n_cols + 1)
// bounds column c of example ex as [ns_off[ex, c], ns_off[ex, c + 1]).
// Slots (unsigned 32-bit arithmetic, M = 2^bits - 1):
//   linear, column c : ((raw + col_seed[c]) & 0x3FFFFFFF) & M
//   pair p = (a, b)  : h = ((raw_i * 16777619) ^ raw_j) & M,
//                      ((h + pair_seed[p]) & 0x3FFFFFFF) & M,
//                      x = __fmul_rn(x_i, x_j)
// Features that share a slot stay separate features on the same atomics.
//
// One 64-lane wave per example, four per block, as in vw_kernels.hip.  Each
// wave stages the first VWI_WINDOW entries of its example in an LDS window of
// its own; every sweep (dot; for --invariant the norm; the update) enumerates
// the features again from the window, entries past it from global memory by
// the same accessor.  Order: linear entries column by column, then pair
// after pair.  Within a pair with |B| >= 64 the lanes run along j for each i;
// with |B| < 64 they stride the flattened i * |B| + j, carried from item to
// item without a divide, so a short side leaves no lane idle.  Per generated
// feature the only global traffic is the gather and the atomics on w, g, s.
// The per-feature arithmetic is vw_sgd_k's, expression for expression.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "vw_device.h"

// 4 windows x 512 x 8 B = 16 KiB per block: eight blocks (the 32 waves a CU
// holds) take 128 KiB of its 160 KiB
#define VWI_WINDOW 512
#define VWI_WAVES 4
#define VWI_MAX_PAIRS 16
#define VWI_FNV 16777619u

// One example as a wave sees it.  k is an entry's position in the example.
struct VwiExample {
  const int* l_idx;    // LDS window
  const float* l_val;
  const int* g_idx;    // global, at the example's first entry
  const float* g_val;
  const long* off;     // the example's n_cols + 1 column bounds
  long base;           // off[0]
  __device__ __forceinline__ unsigned raw(int k) const {
    return (unsigned)(k < VWI_WINDOW ? l_idx[k] : g_idx[k]);
  }
  __device__ __forceinline__ float x(int k) const {
    return k < VWI_WINDOW ? l_val[k] : g_val[k];
  }
};

// f(slot, x) for every feature of the example that falls to this lane.
// pairs (LDS): a, b, seed per pair.
template <class F>
__device__ __forceinline__ void vwi_for_each(
    const VwiExample& e, const int* __restrict__ col_seed, int n_cols,
    const int* pairs, int n_pairs, unsigned mask, int lane, F&& f) {
  for (int c = 0; c < n_cols; ++c) {
    const int s = (int)(e.off[c] - e.base), t = (int)(e.off[c + 1] - e.base);
    const unsigned seed = (unsigned)col_seed[c];
    for (int k = s + lane; k < t; k += WAVE)
      f((int)(((e.raw(k) + seed) & 0x3FFFFFFFu) & mask), e.x(k));
  }
  for (int p = 0; p < n_pairs; ++p) {
    const int a = pairs[3 * p], b = pairs[3 * p + 1];
    const unsigned seed = (unsigned)pairs[3 * p + 2];
    if ((unsigned)a >= (unsigned)n_cols || (unsigned)b >= (unsigned)n_cols)
      continue;
    const int a0 = (int)(e.off[a] - e.base), b0 = (int)(e.off[b] - e.base);
    const int nA = (int)(e.off[a + 1] - e.off[a]);
    const int nB = (int)(e.off[b + 1] - e.off[b]);
    if (nA <= 0 || nB <= 0) continue;
    if (nB < WAVE) {
      // item t = i * nB + j, t = lane, lane + 64, ...: 64 = q * nB + r
      const int q = WAVE / nB, r = WAVE - q * nB;
      int i = lane / nB, j = lane - i * nB;
      while (i < nA) {
        const unsigned h = ((e.raw(a0 + i) * VWI_FNV) ^ e.raw(b0 + j)) & mask;
        f((int)(((h + seed) & 0x3FFFFFFFu) & mask),
          __fmul_rn(e.x(a0 + i), e.x(b0 + j)));
        i += q;
        j += r;
        if (j >= nB) { j -= nB; ++i; }
      }
    } else {
      for (int i = 0; i < nA; ++i) {
        const unsigned hi = e.raw(a0 + i) * VWI_FNV;
        const float xi = e.x(a0 + i);
        for (int j = lane; j < nB; j += WAVE) {
          const unsigned h = (hi ^ e.raw(b0 + j)) & mask;
          f((int)(((h + seed) & 0x3FFFFFFFu) & mask),
            __fmul_rn(xi, e.x(b0 + j)));
        }
      }
    }
  }
}

// Block prologue: pair descriptors into LDS, once.
__device__ __forceinline__ void vwi_stage_pairs(
    int* s_pairs, const int* __restrict__ pairs,
    const int* __restrict__ pair_seed, int n_pairs) {
  for (int p = threadIdx.x; p < n_pairs; p += blockDim.x) {
    s_pairs[3 * p] = pairs[2 * p];
    s_pairs[3 * p + 1] = pairs[2 * p + 1];
    s_pairs[3 * p + 2] = pair_seed[p];
  }
  __syncthreads();
}

// The wave copies the head of its example into its window.  Only this wave
// reads or writes the window, and a wave's LDS operations complete in order,
// so a wave-scope fence is all the ordering it needs.
__device__ __forceinline__ VwiExample vwi_stage(
    int* l_idx, float* l_val, const int* __restrict__ idx,
    const float* __restrict__ val, const long* __restrict__ ns_off,
    int n_cols, long ex, int lane) {
  VwiExample e;
  e.off = ns_off + ex * (n_cols + 1);
  e.base = e.off[0];
  e.g_idx = idx + e.base;
  e.g_val = val + e.base;
  e.l_idx = l_idx;
  e.l_val = l_val;
  const long n = e.off[n_cols] - e.base;
  const int head = (int)(n < VWI_WINDOW ? n : VWI_WINDOW);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (int k = lane; k < head; k += WAVE) {
    l_idx[k] = e.g_idx[k];
    l_val[k] = e.g_val[k];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return e;
}

// eight waves per SIMD (64 VGPRs): the occupancy the window is sized for
__global__ __launch_bounds__(VWI_WAVES * WAVE)
__attribute__((amdgpu_waves_per_eu(8, 8))) void vw_sgd_interact_k(
    const int* __restrict__ idx, const float* __restrict__ val,
    const long* __restrict__ ns_off, const int* __restrict__ col_seed,
    int n_cols, const int* __restrict__ pairs,
    const int* __restrict__ pair_seed, int n_pairs, unsigned mask,
    const float* __restrict__ label, const float* __restrict__ ex_weight,
    float* __restrict__ w_tbl, float* __restrict__ g_tbl,
    float* __restrict__ s_tbl, float lr, float l2, float power_t, int loss,
    int invariant, long n_ex, float* __restrict__ preds_out) {
  __shared__ int s_idx[VWI_WAVES][VWI_WINDOW];
  __shared__ float s_val[VWI_WAVES][VWI_WINDOW];
  __shared__ int s_pairs[3 * VWI_MAX_PAIRS];
  vwi_stage_pairs(s_pairs, pairs, pair_seed, n_pairs);
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const long n_waves = (long)gridDim.x * VWI_WAVES;
  for (long ex = (long)blockIdx.x * VWI_WAVES + wave; ex < n_ex;
       ex += n_waves) {
    const VwiExample e = vwi_stage(s_idx[wave], s_val[wave], idx, val, ns_off,
                                   n_cols, ex, lane);
    float dot = 0.0f;
    vwi_for_each(e, col_seed, n_cols, s_pairs, n_pairs, mask, lane,
                 [&](int i, float x) { dot += w_tbl[i] * x; });
    const float pred = wave_sum(dot);
    if (preds_out && lane == 0) preds_out[ex] = pred;
    const float y = label[ex];
    const float h = ex_weight ? ex_weight[ex] : 1.0f;
    const float gl = dloss(loss, pred, y) * h;
    if (invariant) {
      // sweep 2: sensitivity x_norm = sum x_i^2 * scale_i with the same
      // per-coordinate scales the update will use (G + x^2 proxy)
      float xn = 0.0f;
      vwi_for_each(e, col_seed, n_cols, s_pairs, n_pairs, mask, lane,
                   [&](int i, float x) {
        float sc;
        const float Gp = g_tbl[i] + x * x;
        if (power_t == 0.5f) sc = __frsqrt_rn(Gp + 1e-10f);
        else sc = __powf(Gp + 1e-10f, -power_t);
        if (s_tbl) {
          const float ax = fabsf(x);
          atomicMax((int*)&s_tbl[i], __float_as_int(ax));
          const float sn = fmaxf(__int_as_float(((const int*)s_tbl)[i]), ax);
          if (sn > 0.0f) sc /= sn;
        }
        xn += x * x * sc;
      });
      const float x_norm = wave_sum(xn);
      if (x_norm <= 0.0f) continue;
      const float dp = invariant_dp(loss, pred, y, h * lr * x_norm);
      const float kk = dp / x_norm;
      vwi_for_each(e, col_seed, n_cols, s_pairs, n_pairs, mask, lane,
                   [&](int i, float x) {
        float sc;
        const float Gp = g_tbl[i] + x * x;
        if (power_t == 0.5f) sc = __frsqrt_rn(Gp + 1e-10f);
        else sc = __powf(Gp + 1e-10f, -power_t);
        if (s_tbl) {
          const float sn = fmaxf(__int_as_float(((const int*)s_tbl)[i]),
                                 fabsf(x));
          if (sn > 0.0f) sc /= sn;
        }
        const float g = gl * x + l2 * w_tbl[i];
        atomicAdd(&w_tbl[i], (kk * x - lr * l2 * w_tbl[i]) * sc);
        atomicAdd(&g_tbl[i], g * g);
      });
      continue;
    }
    if (gl == 0.0f) continue;
    vwi_for_each(e, col_seed, n_cols, s_pairs, n_pairs, mask, lane,
                 [&](int i, float x) {
      float g = gl * x + l2 * w_tbl[i];
      const float Gold = atomicAdd(&g_tbl[i], g * g);
      const float G = Gold + g * g;
      // adaptive per-weight rate: lr * G^(-power_t); power_t=0.5 → rsqrt
      float scale;
      if (power_t == 0.5f) scale = __frsqrt_rn(G + 1e-10f);
      else scale = __powf(G + 1e-10f, -power_t);
      if (s_tbl) {  // --normalized: divide by running max|x| per weight
        const float ax = fabsf(x);
        atomicMax((int*)&s_tbl[i], __float_as_int(ax));
        const float sn = fmaxf(__int_as_float(((const int*)s_tbl)[i]), ax);
        if (sn > 0.0f) scale /= sn;
      }
      atomicAdd(&w_tbl[i], -lr * g * scale);
    });
  }
}

__global__ __launch_bounds__(VWI_WAVES * WAVE) void vw_predict_interact_k(
    const int* __restrict__ idx, const float* __restrict__ val,
    const long* __restrict__ ns_off, const int* __restrict__ col_seed,
    int n_cols, const int* __restrict__ pairs,
    const int* __restrict__ pair_seed, int n_pairs, unsigned mask,
    const float* __restrict__ w_tbl, long n_ex, float* __restrict__ out) {
  __shared__ int s_idx[VWI_WAVES][VWI_WINDOW];
  __shared__ float s_val[VWI_WAVES][VWI_WINDOW];
  __shared__ int s_pairs[3 * VWI_MAX_PAIRS];
  vwi_stage_pairs(s_pairs, pairs, pair_seed, n_pairs);
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const long n_waves = (long)gridDim.x * VWI_WAVES;
  for (long ex = (long)blockIdx.x * VWI_WAVES + wave; ex < n_ex;
       ex += n_waves) {
    const VwiExample e = vwi_stage(s_idx[wave], s_val[wave], idx, val, ns_off,
                                   n_cols, ex, lane);
    float dot = 0.0f;
    vwi_for_each(e, col_seed, n_cols, s_pairs, n_pairs, mask, lane,
                 [&](int i, float x) { dot += w_tbl[i] * x; });
    const float pred = wave_sum(dot);
    if (lane == 0) out[ex] = pred;
  }
}

// ---------------------------------------------------------------- launchers
extern "C" int vw_interact_window() { return VWI_WINDOW; }
extern "C" int vw_interact_max_pairs() { return VWI_MAX_PAIRS; }

static unsigned vwi_blocks(long n_ex) {
  long blocks = (n_ex + VWI_WAVES - 1) / VWI_WAVES;
  return (unsigned)(blocks > 4096 ? 4096 : blocks);
}

// Both return -1 (and launch nothing) for more pairs than VWI_MAX_PAIRS.
extern "C" int launch_vw_sgd_interact(
    const int* idx, const float* val, const long* ns_off, const int* col_seed,
    int n_cols, const int* pairs, const int* pair_seed, int n_pairs, int bits,
    const float* label, const float* ex_weight, float* w_tbl, float* g_tbl,
    float* s_tbl, float lr, float l2, float power_t, int loss, int invariant,
    long n_ex, float* preds_out, hipStream_t stream) {
  if (n_pairs > VWI_MAX_PAIRS) return -1;
  if (n_ex == 0) return 0;
  hipLaunchKernelGGL(vw_sgd_interact_k, dim3(vwi_blocks(n_ex)),
                     dim3(VWI_WAVES * WAVE), 0, stream, idx, val, ns_off,
                     col_seed, n_cols, pairs, pair_seed, n_pairs,
                     (1u << bits) - 1u, label, ex_weight, w_tbl, g_tbl, s_tbl,
                     lr, l2, power_t, loss, invariant, n_ex, preds_out);
  return (int)hipGetLastError();
}

extern "C" int launch_vw_predict_interact(
    const int* idx, const float* val, const long* ns_off, const int* col_seed,
    int n_cols, const int* pairs, const int* pair_seed, int n_pairs, int bits,
    const float* w_tbl, long n_ex, float* out, hipStream_t stream) {
  if (n_pairs > VWI_MAX_PAIRS) return -1;
  if (n_ex == 0) return 0;
  hipLaunchKernelGGL(vw_predict_interact_k, dim3(vwi_blocks(n_ex)),
                     dim3(VWI_WAVES * WAVE), 0, stream, idx, val, ns_off,
                     col_seed, n_cols, pairs, pair_seed, n_pairs,
                     (1u << bits) - 1u, w_tbl, n_ex, out);
  return (int)hipGetLastError();
}
