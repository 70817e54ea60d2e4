// Isolation-forest training for gfx950 (MI355X): one block grows one tree.
//
// The forest is the one ops/cpu_ref.py::iforest_build defines, bit for bit:
// every random number is a counter-based hash of (seed, tree, purpose, path,
// draw), rows are sampled through a keyed Feistel bijection, and a node is
// named by its heap path, so nothing depends on scheduling or on the order of
// ids inside a segment.
//
// iforest_build_k<STAGED>   grid = n_trees, 256 threads (4 waves).
//   The tree's subsample lives in LDS as a ping-pong pair of id arrays; a
//   node owns a contiguous segment of positions.  The tree is grown level by
//   level, all nodes of the level at once:
//     sample     every thread evaluates the row bijection (or the bootstrap
//                draw) for its slots;
//     rounds     up to 8 candidate features per unresolved node: every live
//                position loads its value, lanes of a wave that share a node
//                reduce min/max with a segmented shuffle reduction, and the
//                head lane of each run issues ONE LDS atomic min / max on
//                order-preserving uint keys (never sub_n atomics on the
//                root's cell);
//     threshold  one thread per node, unfused round-to-nearest arithmetic;
//     partition  ballot + popcount inside the run, one LDS atomicAdd per run
//                and side on the node's two cursors; left ids fill the
//                segment from the front, right ids from the back;
//     emit       a block prefix sum over the active table numbers the
//                children in level order, writes this level's nodes to the
//                tree's slab of 2 * sub_n - 1 nodes and builds the next
//                level's table; children of size <= 1 or at the height limit
//                are written as leaves at once, so at most sub_n / 2 nodes
//                are ever active.
//   STAGED (sub_n * nf <= 8192): the sample is copied once into LDS,
//   feature-major Xs[f * sub_n + slot], ids are slots and every level reads
//   LDS only.  Otherwise ids are row numbers and each pass gathers
//   X[row * nf + f] from global memory (L2).
//
//   LDS, S = sub_n, T = max(S / 2, 1), all dynamic:
//     ids 2 * 4S, node-of-position 2S, table 9 * 4T, scan scratch 32 B,
//     staged sample 4 * S * nf <= 32 KB.
//   At the limit S = 4096: 32768 + 8192 + 73728 + 32 = 114720 B gathered,
//   147488 B staged, below gfx950's 160 KB per block; the launcher raises the
//   dynamic limit above 64 KB.  At the default S = 256: 7.2 KB + sample.
//
// iforest_compact_k         grid = n_trees: copies each slab's used prefix to
//   its compact offset (offsets = cumsum of the node counts).
#include <hip/hip_runtime.h>
#include <cstdint>

#define IF_THREADS 256
#define IF_MAX_SUB 4096
#define IF_STAGE_MAX 8192
#define IF_RETRIES 8
#define IF_NONE 0xFFFFu
#define IF_RESOLVED 0x100u
#define IF_GOLD 0x9E3779B97F4A7C15ull

enum { IF_ROWPERM = 0, IF_BOOT = 1, IF_FEATPERM = 2, IF_NODE_FEAT = 3,
       IF_NODE_THR = 4 };

__device__ __forceinline__ uint64_t if_fin(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// kt = the hash after (seed, tree); the three remaining fields fold in here
__device__ __forceinline__ uint64_t if_mix(uint64_t kt, uint64_t purpose,
                                           uint64_t path, uint64_t draw) {
  uint64_t h = if_fin((kt ^ purpose) + IF_GOLD);
  h = if_fin((h ^ path) + IF_GOLD);
  return if_fin((h ^ draw) + IF_GOLD);
}

__device__ __forceinline__ uint32_t if_below(uint64_t h, uint32_t m) {
  return (uint32_t)(((h >> 32) * (uint64_t)m) >> 32);
}

// 4-round Feistel on 2^(2 * half) values, cycle-walked back below n
__device__ __forceinline__ uint32_t if_perm(uint64_t kt, uint64_t purpose,
                                            uint32_t x, uint32_t n, int half) {
  const uint32_t mask = (1u << half) - 1u;
  do {
    uint32_t L = x >> half, R = x & mask;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t F = (uint32_t)(if_mix(kt, purpose, r, R) >> 32) & mask;
      const uint32_t nr = L ^ F;
      L = R;
      R = nr;
    }
    x = (L << half) | R;
  } while (x >= n);
  return x;
}

__device__ __forceinline__ uint32_t if_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float if_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// thr = lo + u * (hi - lo) with one rounding per operation, clamped into
// (lo, hi].  Plain operators with contraction switched off: the headers'
// __fmul_rn / __fadd_rn are themselves `x * y` and `x + y` compiled under
// the default fp-contract=fast, and were fused into one v_fma_f32 here.
__device__ __forceinline__ float if_threshold(float lo, float hi, float u) {
#pragma clang fp contract(off)
  const float span = hi - lo;
  const float step = u * span;
  float thr = lo + step;
  thr = thr < hi ? thr : hi;
  return thr > lo ? thr : hi;
}

struct IfLds {
  int* ids;             // 2 x S: slots (staged) or row numbers, ping-pong
  uint32_t* seg;        // 2 x T: start | len << 16, ping-pong
  uint32_t* pi;         // 2 x T: heap path | output node index << 16
  int* feat;            // T: candidate, then chosen, feature
  uint32_t* state;      // T: draw being tried; | IF_RESOLVED; IF_RETRIES = leaf
  uint32_t* ka;         // T: min key, then the threshold's bits
  uint32_t* kb;         // T: max key, then the left cursor (= left count)
  uint32_t* rc;         // T: right cursor, then child table indices l | r << 16
  uint32_t* scan;       // 8: wave totals of the block scan
  uint16_t* nodeof;     // S: table index of each position, IF_NONE = retired
  float* xs;            // staged sample, feature-major
};

__device__ __forceinline__ IfLds if_carve(unsigned char* base, int S, int T) {
  IfLds l;
  uint32_t* w = (uint32_t*)base;
  l.ids = (int*)w; w += 2 * S;
  l.seg = w; w += 2 * T;
  l.pi = w; w += 2 * T;
  l.feat = (int*)w; w += T;
  l.state = w; w += T;
  l.ka = w; w += T;
  l.kb = w; w += T;
  l.rc = w; w += T;
  l.scan = w; w += 8;
  l.xs = (float*)w;
  l.nodeof = nullptr;             // the 16-bit array goes last, after xs
  return l;
}

static size_t if_lds_bytes(int S, int nf, bool staged) {
  const size_t T = S / 2 > 1 ? S / 2 : 1;
  size_t b = 4 * (2 * (size_t)S + 9 * T + 8);
  if (staged) b += 4 * (size_t)S * nf;
  return b + 2 * (((size_t)S + 1) & ~(size_t)1);
}

template <bool STAGED>
__global__ __launch_bounds__(IF_THREADS) void iforest_build_k(
    const float* __restrict__ X, uint32_t n, int nf, int S, int n_feat,
    int bootstrap, uint64_t seed, int height, int half_n, int half_f,
    int* __restrict__ sample_rows, int* __restrict__ o_feature,
    float* __restrict__ o_threshold, int* __restrict__ o_left,
    int* __restrict__ o_right, int* __restrict__ o_size,
    int* __restrict__ o_depth, int* __restrict__ o_count) {
  extern __shared__ __align__(16) unsigned char if_smem[];
  const int T = S / 2 > 1 ? S / 2 : 1;
  IfLds l = if_carve(if_smem, S, T);
  l.nodeof = (uint16_t*)(l.xs + (STAGED ? (size_t)S * nf : 0));

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t tree = blockIdx.x;
  const uint64_t kt = if_fin((if_fin(seed + IF_GOLD) ^ (uint64_t)tree) + IF_GOLD);
  const size_t slab = (size_t)tree * (2 * (size_t)S - 1);
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  const uint64_t le_mask = (2ull << lane) - 1ull;   // lane 63: all ones

  // ---- sample
  for (int s = tid; s < S; s += IF_THREADS) {
    const uint32_t row = bootstrap
        ? if_below(if_mix(kt, IF_BOOT, 0, (uint64_t)s), n)
        : if_perm(kt, IF_ROWPERM, (uint32_t)s, n, half_n);
    sample_rows[(size_t)tree * S + s] = (int)row;
    l.ids[s] = STAGED ? s : (int)row;
    l.nodeof[s] = 0;
    if (STAGED) {
      const float* xr = X + (size_t)row * nf;
      for (int f = 0; f < nf; ++f) l.xs[f * S + s] = xr[f];
    }
  }
  if (tid == 0) {
    l.seg[0] = (uint32_t)S << 16;
    l.pi[0] = 1u;
  }
  int m = 1, next_out = 1, cur = 0;
  __syncthreads();

  for (int d = 0; m > 0; ++d) {
    const int* ids = l.ids + cur * S;
    int* ids_nxt = l.ids + (cur ^ 1) * S;
    const uint32_t* seg = l.seg + cur * T;
    const uint32_t* pi = l.pi + cur * T;

    for (int j = tid; j < m; j += IF_THREADS) {
      l.state[j] = 0u;
      l.ka[j] = 0xFFFFFFFFu;
      l.kb[j] = 0u;
    }
    __syncthreads();

    // ---- candidate rounds over the unresolved nodes
    for (int r = 0; r < IF_RETRIES; ++r) {
      int pending = 0;
      for (int j = tid; j < m; j += IF_THREADS) {
        if (l.state[j] == (uint32_t)r) {
          uint32_t f = if_below(
              if_mix(kt, IF_NODE_FEAT, pi[j] & 0xFFFFu, (uint64_t)r),
              (uint32_t)n_feat);
          if (n_feat < nf) f = if_perm(kt, IF_FEATPERM, f, (uint32_t)nf, half_f);
          l.feat[j] = (int)f;
          pending = 1;
        }
      }
      if (!__syncthreads_or(pending)) break;

      for (int p0 = wave * 64; p0 < S; p0 += IF_THREADS) {
        const int p = p0 + lane;
        uint32_t j = p < S ? l.nodeof[p] : IF_NONE;
        if (j != IF_NONE && l.state[j] != (uint32_t)r) j = IF_NONE;
        if (__ballot(j != IF_NONE) == 0ull) continue;
        uint32_t kmn = 0xFFFFFFFFu, kmx = 0u;
        if (j != IF_NONE) {
          const int f = l.feat[j], id = ids[p];
          const float v = STAGED ? l.xs[f * S + id]
                                 : X[(size_t)id * nf + f];
          kmn = kmx = if_key(v);
        }
        // runs of one node are contiguous lanes: a doubling scan that only
        // combines equal nodes leaves the run's result in its head lane
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const uint32_t oj = __shfl_down(j, off, 64);
          const uint32_t omn = __shfl_down(kmn, off, 64);
          const uint32_t omx = __shfl_down(kmx, off, 64);
          if (lane + off < 64 && oj == j) {
            kmn = omn < kmn ? omn : kmn;
            kmx = omx > kmx ? omx : kmx;
          }
        }
        const uint32_t pj = __shfl_up(j, 1, 64);
        if (j != IF_NONE && (lane == 0 || pj != j)) {
          atomicMin(&l.ka[j], kmn);
          atomicMax(&l.kb[j], kmx);
        }
      }
      __syncthreads();

      for (int j = tid; j < m; j += IF_THREADS) {
        if (l.state[j] == (uint32_t)r) {
          if (if_unkey(l.kb[j]) > if_unkey(l.ka[j])) {
            l.state[j] = (uint32_t)r | IF_RESOLVED;
          } else {
            l.state[j] = (uint32_t)r + 1u;
            l.ka[j] = 0xFFFFFFFFu;
            l.kb[j] = 0u;
          }
        }
      }
      __syncthreads();
    }

    // ---- thresholds; ka becomes thr, kb and rc the two cursors
    for (int j = tid; j < m; j += IF_THREADS) {
      const uint32_t st = l.state[j];
      if (st & IF_RESOLVED) {
        const float lo = if_unkey(l.ka[j]), hi = if_unkey(l.kb[j]);
        const uint64_t h = if_mix(kt, IF_NODE_THR, pi[j] & 0xFFFFu,
                                  (uint64_t)(st & 0xFFu));
        const float u = (float)(uint32_t)(h >> 40) * 0x1p-24f;   // exact
        l.ka[j] = __float_as_uint(if_threshold(lo, hi, u));
      }
      l.kb[j] = 0u;
      l.rc[j] = 0u;
    }
    __syncthreads();

    // ---- partition every resolved segment into the other id buffer
    for (int p0 = wave * 64; p0 < S; p0 += IF_THREADS) {
      const int p = p0 + lane;
      uint32_t j = p < S ? l.nodeof[p] : IF_NONE;
      if (j != IF_NONE && !(l.state[j] & IF_RESOLVED)) j = IF_NONE;
      const uint64_t act = __ballot(j != IF_NONE);
      if (act == 0ull) continue;
      int id = 0;
      bool gl = false;
      if (j != IF_NONE) {
        const int f = l.feat[j];
        id = ids[p];
        const float v = STAGED ? l.xs[f * S + id] : X[(size_t)id * nf + f];
        gl = v < __uint_as_float(l.ka[j]);
      }
      const uint32_t pj = __shfl_up(j, 1, 64);
      const uint64_t heads = __ballot(lane == 0 || pj != j);
      const int run_start = 63 - __clzll((long long)(heads & le_mask));
      const uint64_t above = heads & ~le_mask;
      const int run_end = above ? __ffsll((long long)above) - 2 : 63;
      const uint64_t run = ((2ull << run_end) - 1ull) & ~((1ull << run_start) - 1ull);
      const uint64_t glb = __ballot(gl);
      const uint64_t lmask = glb & run, rmask = act & ~glb & run;
      uint32_t bl = 0u, br = 0u;
      if (j != IF_NONE && lane == run_start) {
        bl = atomicAdd(&l.kb[j], (uint32_t)__popcll(lmask));
        br = atomicAdd(&l.rc[j], (uint32_t)__popcll(rmask));
      }
      bl = __shfl(bl, run_start, 64);
      br = __shfl(br, run_start, 64);
      if (j != IF_NONE) {
        const uint32_t sg = seg[j], start = sg & 0xFFFFu, len = sg >> 16;
        const uint32_t dest = gl
            ? start + bl + (uint32_t)__popcll(lmask & lt_mask)
            : start + len - 1u - (br + (uint32_t)__popcll(rmask & lt_mask));
        ids_nxt[dest] = id;
      }
    }
    __syncthreads();

    // ---- emit the level, number the children, build the next table
    const int chunk = (m + IF_THREADS - 1) / IF_THREADS;
    const int j0 = tid * chunk, j1 = min(m, j0 + chunk);
    uint32_t mine = 0u;           // resolved nodes | active children << 16
    for (int j = j0; j < j1; ++j) {
      if (l.state[j] & IF_RESOLVED) {
        const uint32_t len = seg[j] >> 16, lc = l.kb[j], rn = len - lc;
        const bool deeper = d + 1 < height;
        mine += 1u + ((uint32_t)(deeper && lc > 1u) << 16)
                + ((uint32_t)(deeper && rn > 1u) << 16);
      }
    }
    uint32_t incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    if (lane == 63) l.scan[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
    for (int w = 0; w < IF_THREADS / 64; ++w) {
      const uint32_t s = l.scan[w];
      if (w < wave) before += s;
      total += s;
    }
    uint32_t excl = before + incl - mine;
    uint32_t ri = excl & 0xFFFFu, oa = excl >> 16;
    uint32_t* seg_nxt = l.seg + (cur ^ 1) * T;
    uint32_t* pi_nxt = l.pi + (cur ^ 1) * T;
    for (int j = j0; j < j1; ++j) {
      const uint32_t sg = seg[j], start = sg & 0xFFFFu, len = sg >> 16;
      const uint32_t path = pi[j] & 0xFFFFu, out = pi[j] >> 16;
      const bool res = l.state[j] & IF_RESOLVED;
      o_size[slab + out] = (int)len;
      o_depth[slab + out] = d;
      if (!res) {
        o_feature[slab + out] = -1;
        o_threshold[slab + out] = 0.0f;
        o_left[slab + out] = -1;
        o_right[slab + out] = -1;
        continue;
      }
      const uint32_t lc = l.kb[j];
      const uint32_t L = (uint32_t)next_out + 2u * ri;
      ++ri;
      o_feature[slab + out] = l.feat[j];
      o_threshold[slab + out] = __uint_as_float(l.ka[j]);
      o_left[slab + out] = (int)L;
      o_right[slab + out] = (int)L + 1;
      uint32_t ct[2];
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const uint32_t clen = side ? len - lc : lc;
        const uint32_t cstart = side ? start + lc : start;
        const uint32_t cout = L + side;
        if (clen > 1u && d + 1 < height) {
          seg_nxt[oa] = cstart | (clen << 16);
          pi_nxt[oa] = (2u * path + side) | (cout << 16);
          ct[side] = oa++;
        } else {
          o_feature[slab + cout] = -1;
          o_threshold[slab + cout] = 0.0f;
          o_left[slab + cout] = -1;
          o_right[slab + cout] = -1;
          o_size[slab + cout] = (int)clen;
          o_depth[slab + cout] = d + 1;
          ct[side] = IF_NONE;
        }
      }
      l.rc[j] = ct[0] | (ct[1] << 16);
    }
    __syncthreads();

    // ---- positions learn their child's table index
    for (int p = tid; p < S; p += IF_THREADS) {
      const uint32_t j = l.nodeof[p];
      if (j == IF_NONE) continue;
      uint32_t c = IF_NONE;
      if (l.state[j] & IF_RESOLVED) {
        const uint32_t start = seg[j] & 0xFFFFu;
        c = (uint32_t)p < start + l.kb[j] ? (l.rc[j] & 0xFFFFu)
                                          : (l.rc[j] >> 16);
      }
      l.nodeof[p] = (uint16_t)c;
    }
    next_out += 2 * (int)(total & 0xFFFFu);
    m = (int)(total >> 16);
    cur ^= 1;
    __syncthreads();
  }
  if (tid == 0) o_count[tree] = next_out;
}

__global__ __launch_bounds__(IF_THREADS) void iforest_compact_k(
    const int* __restrict__ s_feature, const float* __restrict__ s_threshold,
    const int* __restrict__ s_left, const int* __restrict__ s_right,
    const int* __restrict__ s_size, const int* __restrict__ s_depth,
    const long* __restrict__ offsets, int cap, int* __restrict__ feature,
    float* __restrict__ threshold, int* __restrict__ left,
    int* __restrict__ right, int* __restrict__ size, int* __restrict__ depth) {
  const long base = offsets[blockIdx.x];
  const int cnt = (int)(offsets[blockIdx.x + 1] - base);
  const size_t slab = (size_t)blockIdx.x * cap;
  for (int i = threadIdx.x; i < cnt && i < cap; i += IF_THREADS) {
    feature[base + i] = s_feature[slab + i];
    threshold[base + i] = s_threshold[slab + i];
    left[base + i] = s_left[slab + i];
    right[base + i] = s_right[slab + i];
    size[base + i] = s_size[slab + i];
    depth[base + i] = s_depth[slab + i];
  }
}

extern "C" int iforest_max_sub() { return IF_MAX_SUB; }

// 1 when the launcher stages the tree's sample in LDS
extern "C" int iforest_staged(int sub_n, int nf) {
  return (long)sub_n * nf <= IF_STAGE_MAX;
}

static int if_half_bits(unsigned long n) {
  int b = 2;
  while ((1ul << b) < n) ++b;
  return (b + 1) / 2;
}

extern "C" int launch_iforest_build(
    const float* X, long n, int nf, int n_trees, int sub_n, int n_feat,
    int bootstrap, unsigned long long seed, int* sample_rows, int* feature,
    float* threshold, int* left, int* right, int* size, int* depth,
    int* count, hipStream_t stream) {
  if (n < 2 || n >= (1L << 31) || sub_n < 2 || sub_n > IF_MAX_SUB ||
      sub_n > n || nf < 1 || n_feat < 1 || n_feat > nf || n_trees < 1)
    return (int)hipErrorInvalidValue;
  int height = 0;
  while ((1 << height) < sub_n) ++height;
  const bool staged = iforest_staged(sub_n, nf);
  const size_t lds = if_lds_bytes(sub_n, nf, staged);
  auto kern = staged ? iforest_build_k<true> : iforest_build_k<false>;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(
        (const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3(n_trees), dim3(IF_THREADS), lds, stream, X,
                     (uint32_t)n, nf, sub_n, n_feat, bootstrap,
                     (uint64_t)seed, height, if_half_bits((unsigned long)n),
                     if_half_bits((unsigned long)nf), sample_rows, feature,
                     threshold, left, right, size, depth, count);
  return (int)hipGetLastError();
}

extern "C" int launch_iforest_compact(
    const int* s_feature, const float* s_threshold, const int* s_left,
    const int* s_right, const int* s_size, const int* s_depth,
    const long* offsets, int n_trees, int cap, int* feature, float* threshold,
    int* left, int* right, int* size, int* depth, hipStream_t stream) {
  hipLaunchKernelGGL(iforest_compact_k, dim3(n_trees), dim3(IF_THREADS), 0,
                     stream, s_feature, s_threshold, s_left, s_right, s_size,
                     s_depth, offsets, cap, feature, threshold, left, right,
                     size, depth);
  return (int)hipGetLastError();
}
