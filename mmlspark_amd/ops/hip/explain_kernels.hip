// Coalition values of GBDT forests for KernelSHAP and LIME on MI355X (gfx950):
// the perturbed samples states*x + (1-states)*background never exist.  The
// forest walk picks every feature value at the node that tests it: bit f of the
// coalition mask selects the explained row's x[f] or the drawn background row's
// bg[b][f].  Matrix instructions have no place here: this is a gather-and-
// branch kernel, one dependent LDS read per tree level.
//
//   coalition_values_k  grid = (item blocks, explained rows).  A workgroup of
//       256 threads serves ONE explained row; the row sits in LDS, so the
//       common side of every select is an LDS read, and the background side is
//       a global read of a table that is L2-resident at explainer sizes.
//       Work is cut over (coalition, draw segment) ITEMS, not over coalitions:
//       the B draws of a coalition are cut into `dsplit` contiguous segments
//       of seg_len draws and item = coalition * dsplit + segment, so 30
//       coalitions x 1000 cycled draws fill the device as 10,000 x 1 does.  A
//       thread owns one item.  Its mask lives in a register when nf <= 32 and
//       otherwise in LDS as [word][thread] (conflict-free); masks are read
//       from global memory once.
//       The forest moves through LDS in tiles of WHOLE trees.  The block finds
//       a tile's last tree itself (thread j tests tree ts+1+j against the node
//       budget, an LDS integer max joins them; at most 256 trees per tile) and
//       packs each node into 16 bytes while staging, so a node is one aligned
//       ds_read_b128:
//           x = threshold bits | leaf value bits | category-set offset
//           y = feature (clamped to nf-1), bit 30 = categorical; -1 = leaf
//           z, w = left, right child, relative to the tree's first node
//       Every thread walks the staged tile before the next tile is loaded; a tree that exceeds the tile is walked from the flat
//       arrays in global memory by the same code.  If the tree range is one
//       tile it is staged once and kept for every draw.
//       Raw sums are float32 registers, K of them, started at base[k] and
//       advanced by fmaf(weight, leaf, sum) in tree order: n - 1 roundings for
//       the n = t1 - t0 + 1 terms.  The transform (identity, binary sigmoid,
//       softmax) is evaluated in float64 and added to a float64 accumulator:
//       one double add per forest traversal, draws of a segment in draw order.
//   coalition_merge_k  only when dsplit > 1: one thread per (row, coalition,
//       class) adds the segments' partial sums in segment order and divides by
//       B.  With dsplit == 1 the first kernel divides and stores itself.
//
// No floating-point atomics, and dsplit and the tile size depend on the
// shapes alone, so a call is bit-repeatable.  With exactly summable leaves
// the identity output is numpy's float64 mean, bit for bit, for every tile
// size.  Node tests are go_left_node's of gbdt_kernels.hip, with one
// difference: a category value in [255.5, 256) rounds to 256, for which
// go_left_node reads the word after the node's 256-bit set; here it is
// clamped to category 255, as cpu_ref._go_left clamps it.
#include <hip/hip_runtime.h>

#define EXPLAIN_MAX_FEATURES 256
#define EXPLAIN_MAX_OUTPUTS 8
#define EXPLAIN_MAX_TILE_NODES 6144   // 96 KiB of packed nodes
#define EXPLAIN_TILE_NODES 4096       // default: two workgroups per CU
#define EXPLAIN_THREADS 256
#define EXPLAIN_MAX_W (EXPLAIN_MAX_FEATURES / 32)
#define EXPLAIN_CAT_BIT 0x40000000
#define EXPLAIN_FILL_THREADS 131072   // 256 CUs x 512 threads

enum { EXPLAIN_IDENTITY = 0, EXPLAIN_SIGMOID = 1, EXPLAIN_SOFTMAX = 2 };

struct ExplainForest {
  const int* feat;
  const float* thr;
  const int* left;
  const int* right;
  const float* val;
  const long* offsets;
  const float* tw;
  const int* catoff;       // null: no categorical nodes
  const unsigned* catw;
};

// go_left_node of gbdt_kernels.hip on a packed node.
__device__ __forceinline__ bool explain_go_left(float xv, int4 nd,
                                                const unsigned* catw) {
  if (nd.y & EXPLAIN_CAT_BIT) {
    if (isnan(xv) || xv < 0.0f || xv >= 256.0f) return true;
    const int b = min((int)rintf(xv), 255);  // 255.5 <= xv < 256 rounds to 256
    return (catw[(long)nd.x * 8 + (b >> 5)] >> (b & 31)) & 1u;
  }
  return xv <= __int_as_float(nd.x) || isnan(xv);
}

__device__ __forceinline__ int4 explain_pack_node(const ExplainForest& F,
                                                  long g, int nf) {
  const int f = F.feat[g];
  if (f < 0) return make_int4(__float_as_int(F.val[g]), -1, 0, 0);
  int x = __float_as_int(F.thr[g]);
  int y = min(f, nf - 1);
  if (F.catoff != nullptr) {
    const int off = F.catoff[g];
    if (off >= 0) { x = off; y |= EXPLAIN_CAT_BIT; }
  }
  return make_int4(x, y, F.left[g], F.right[g]);
}

// Walk one tree from its root to a leaf and return the leaf value; `node(i)`
// returns the packed node i of the tree (from the LDS tile or from global
// memory).  `mask` is the coalition's word when MREG, else its words sit in
// LDS at mlds[word * EXPLAIN_THREADS].
template <bool MREG, class NodeAt>
__device__ __forceinline__ float explain_walk_tree(
    NodeAt node, const float* __restrict__ xs, const float* __restrict__ bgp,
    unsigned mask, const unsigned* __restrict__ mlds,
    const unsigned* __restrict__ catw) {
  int4 nd = node(0);
  while (nd.y >= 0) {
    const int f = nd.y & 0xFFFF;
    const unsigned word = MREG ? mask : mlds[(f >> 5) * EXPLAIN_THREADS];
    const float xv = ((word >> (f & 31)) & 1u) ? xs[f] : bgp[f];
    nd = node(explain_go_left(xv, nd, catw) ? nd.z : nd.w);
  }
  return __int_as_float(nd.x);
}

// LDS image (dynamic): [tile_nodes int4 | xs nf floats, padded to 4 |
// masks MAX_W*256 words unless MREG].  Static: tree starts and weights of
// the staged tile, and the tile's end tree.
template <bool MULTI, bool MREG>
__global__ __launch_bounds__(EXPLAIN_THREADS) void coalition_values_k(
    ExplainForest F, int t0, int t1, int K, const float* __restrict__ X,
    const float* __restrict__ bg, int nb, int nf,
    const unsigned* __restrict__ masks, int mask_rows, int W, int nZ,
    const int* __restrict__ bidx, int B, int dsplit, int seg_len,
    const float* __restrict__ base, int transform, float sigmoid,
    const int* __restrict__ classes, int C, int tile_nodes,
    double* __restrict__ dst) {
  constexpr int KM = MULTI ? EXPLAIN_MAX_OUTPUTS : 1;
  constexpr int KA = MULTI ? EXPLAIN_MAX_OUTPUTS : 2;  // binary: p and 1 - p
  extern __shared__ __attribute__((aligned(16))) int4 explain_lds[];
  __shared__ int s_tstart[EXPLAIN_THREADS];
  __shared__ float s_tw[EXPLAIN_THREADS];
  __shared__ int s_te;
  int4* tile = explain_lds;
  float* xs = (float*)(tile + tile_nodes);
  unsigned* mlds = (unsigned*)(xs + ((nf + 3) & ~3)) + threadIdx.x;

  const int tid = threadIdx.x;
  const int r = blockIdx.y;
  const long n_items = (long)nZ * dsplit;
  for (int f = tid; f < nf; f += EXPLAIN_THREADS) xs[f] = X[(long)r * nf + f];

  // the thread's item: coalition, first draw, mask words.  A thread past the
  // last item walks coalition 0 for the barriers' sake and stores nothing.
  const long it = (long)blockIdx.x * EXPLAIN_THREADS + tid;
  const bool live = it < n_items;
  const int z = live ? (int)(it / dsplit) : 0;
  const int d0 = live ? (int)(it % dsplit) * seg_len : 0;
  const unsigned* mrow = masks + ((long)(mask_rows == 1 ? 0 : r) * nZ + z) * W;
  unsigned mask = 0;
  if (MREG) {
    mask = mrow[0];
  } else {
    for (int w = 0; w < W; ++w) mlds[w * EXPLAIN_THREADS] = mrow[w];
  }

  double acc[KA];
#pragma unroll
  for (int k = 0; k < KA; ++k) acc[k] = 0.0;

  int staged = -1;  // first tree of the tile that LDS holds
  for (int j = 0; j < seg_len; ++j) {
    // this pass's draw and its background row
    const int d = d0 + j;
    const bool on = live && d < B;
    int b = 0;
    if (on) b = bidx ? bidx[((long)r * nZ + z) * B + d] : d;
    b = min(max(b, 0), nb - 1);
    const float* bgp = bg + (long)b * nf;
    float raw[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) raw[k] = k < K ? base[k] : 0.0f;

    int ts = t0;
    while (ts < t1) {
      __syncthreads();  // the previous tile's walk and s_te are done with
      if (tid == 0) s_te = ts;
      __syncthreads();
      const long off_ts = F.offsets[ts];
      long off_mine = 0;   // start of tree ts + tid
      if (ts + tid <= t1) off_mine = F.offsets[min(ts + tid, t1)];
      {
        const int cand = ts + 1 + tid;  // tile would end before tree cand
        if (cand <= t1 && F.offsets[cand] - off_ts <= (long)tile_nodes)
          atomicMax(&s_te, cand);
      }
      __syncthreads();
      const int te = s_te;
      if (te == ts) {  // tree ts exceeds the tile: walk it in global memory
        const float leaf = explain_walk_tree<MREG>(
            [&](int i) { return explain_pack_node(F, off_ts + i, nf); }, xs,
            bgp, mask, mlds, F.catw);
        const float w = F.tw[ts];
        const int cls = MULTI ? ts % K : 0;
#pragma unroll
        for (int k = 0; k < KM; ++k)
          if (k == cls) raw[k] = fmaf(w, leaf, raw[k]);
        ts += 1;
        continue;
      }
      if (staged != ts) {
        if (ts + tid < te) {
          s_tstart[tid] = (int)(off_mine - off_ts);
          s_tw[tid] = F.tw[ts + tid];
        }
        const int n_tile = (int)(F.offsets[te] - off_ts);
        for (int i = tid; i < n_tile; i += EXPLAIN_THREADS)
          tile[i] = explain_pack_node(F, off_ts + i, nf);
        staged = ts;
        __syncthreads();
      }
      for (int t = ts; t < te; ++t) {
        const int4* tree = tile + s_tstart[t - ts];
        const float leaf = explain_walk_tree<MREG>(
            [&](int i) { return tree[i]; }, xs, bgp, mask, mlds, F.catw);
        const float w = s_tw[t - ts];
        const int cls = MULTI ? t % K : 0;
#pragma unroll
        for (int k = 0; k < KM; ++k)
          if (k == cls) raw[k] = fmaf(w, leaf, raw[k]);
      }
      ts = te;
    }

    // transform in float64, one double add per traversal
    if (!on) continue;
    if (!MULTI) {
      double v = (double)raw[0];
      if (transform == EXPLAIN_SIGMOID) {
        v = 1.0 / (1.0 + exp(-(double)sigmoid * v));
        acc[1] += v;
        v = 1.0 - v;
      }
      acc[0] += v;
    } else if (transform == EXPLAIN_SOFTMAX) {
      double mx = (double)raw[0];
#pragma unroll
      for (int k = 1; k < KM; ++k)
        if (k < K) mx = fmax(mx, (double)raw[k]);
      double e[KM], sum = 0.0;
#pragma unroll
      for (int k = 0; k < KM; ++k) {
        e[k] = k < K ? exp((double)raw[k] - mx) : 0.0;
        sum += e[k];
      }
#pragma unroll
      for (int k = 0; k < KM; ++k) acc[k] += e[k] / sum;
    } else {
#pragma unroll
      for (int k = 0; k < KM; ++k) acc[k] += (double)raw[k];
    }
  }

  // dsplit == 1: the mean itself to out (R, nZ, C); otherwise the segment's
  // sum to part (R, nZ, dsplit, C).  A binary sigmoid has one raw output and
  // two classes: class 1 is p, class 0 is 1 - p.  A class outside the
  // outputs selects nothing and stores 0.
  if (!live) return;
  double* o = dst + ((long)r * n_items + it) * C;
  for (int c = 0; c < C; ++c) {
    const int cls = classes[c];
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < KA; ++k)
      if (k == cls) v = acc[k];
    o[c] = dsplit == 1 ? v / (double)B : v;
  }
}

__global__ void coalition_merge_k(const double* __restrict__ part, long n,
                                  int dsplit, int C, int B,
                                  double* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (r, z, c)
  if (i >= n) return;
  const long rz = i / C;
  const int c = (int)(i % C);
  double s = 0.0;
  for (int g = 0; g < dsplit; ++g) s += part[(rz * dsplit + g) * C + c];
  out[i] = s / (double)B;
}

// How the draws of a coalition are cut: segments of seg_len draws, enough of
// them that R * nZ * dsplit items reach EXPLAIN_FILL_THREADS.
extern "C" int explain_draw_splits(long R, long nZ, int B) {
  const long rz = R * nZ > 0 ? R * nZ : 1;
  long want = (EXPLAIN_FILL_THREADS + rz - 1) / rz;
  if (want > B) want = B;
  if (want < 1) want = 1;
  const int seg_len = (int)((B + want - 1) / want);
  return (B + seg_len - 1) / seg_len;
}

template <bool MULTI, bool MREG>
static int explain_launch_as(const ExplainForest& F, int t0, int t1, int K,
                             const float* X, long R, const float* bg, int nb,
                             int nf, const unsigned* masks, int mask_rows,
                             int W, int nZ, const int* bidx, int B, int dsplit,
                             int seg_len, const float* base, int transform,
                             float sigmoid, const int* classes, int C,
                             int tile_nodes, double* dst,
                             hipStream_t stream) {
  const long n_items = (long)nZ * dsplit;
  const long blocks = (n_items + EXPLAIN_THREADS - 1) / EXPLAIN_THREADS;
  size_t lds = sizeof(int4) * (size_t)tile_nodes
               + sizeof(float) * (size_t)((nf + 3) & ~3);
  if (!MREG) lds += sizeof(unsigned) * EXPLAIN_MAX_W * EXPLAIN_THREADS;
  auto kern = coalition_values_k<MULTI, MREG>;
  hipError_t err = hipFuncSetAttribute(
      (const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)R),
                     dim3(EXPLAIN_THREADS), lds, stream, F, t0, t1, K, X, bg,
                     nb, nf, masks, mask_rows, W, nZ, bidx, B, dsplit, seg_len,
                     base, transform, sigmoid, classes, C, tile_nodes, dst);
  return (int)hipGetLastError();
}

// out (R, nZ, C) float64; part (R, nZ, dsplit, C) float64 scratch, used only
// when dsplit = explain_draw_splits(R, nZ, B) exceeds 1.  tile_nodes 0 = the
// kernel's policy.  Returns a hipError_t, or -1 for an argument out of range.
extern "C" int launch_coalition_values(
    const int* feat, const float* thr, const int* left, const int* right,
    const float* val, const long* offsets, const float* tw, const int* catoff,
    const unsigned* catw, long total_nodes, int t0, int t1, int K,
    const float* X, long R, const float* bg, int nb, int nf,
    const unsigned* masks, int mask_rows, int nZ, const int* bidx, int B,
    const float* base, int transform, float sigmoid, const int* classes,
    int C, int tile_nodes, double* part, double* out, hipStream_t stream) {
  if (R <= 0 || nZ <= 0 || C <= 0) return 0;
  if (nf < 1 || nf > EXPLAIN_MAX_FEATURES || K < 1 || K > EXPLAIN_MAX_OUTPUTS
      || B < 1 || nb < 1 || R > 65535 || tile_nodes < 0
      || tile_nodes > EXPLAIN_MAX_TILE_NODES)
    return -1;
  if (tile_nodes == 0) {  // no more LDS than the forest can use
    tile_nodes = EXPLAIN_TILE_NODES;
    if (total_nodes < tile_nodes) tile_nodes = (int)(total_nodes > 1 ? total_nodes : 1);
  }
  const int W = (nf + 31) / 32;
  const int dsplit = explain_draw_splits(R, nZ, B);
  const int seg_len = (B + dsplit - 1) / dsplit;
  const ExplainForest F = {feat, thr, left, right, val, offsets, tw, catoff,
                           catw};
  const bool multi = K > 1;
  const bool mreg = W == 1;
  double* dst = dsplit == 1 ? out : part;
#define EXPLAIN_GO(M, G)                                                      \
  explain_launch_as<M, G>(F, t0, t1, K, X, R, bg, nb, nf, masks, mask_rows,   \
                          W, nZ, bidx, B, dsplit, seg_len, base, transform,   \
                          sigmoid, classes, C, tile_nodes, dst, stream)
  int err;
  if (multi) err = mreg ? EXPLAIN_GO(true, true) : EXPLAIN_GO(true, false);
  else err = mreg ? EXPLAIN_GO(false, true) : EXPLAIN_GO(false, false);
#undef EXPLAIN_GO
  if (err != 0 || dsplit == 1) return err;
  const long n = R * (long)nZ * C;
  hipLaunchKernelGGL(coalition_merge_k, dim3((unsigned)((n + 255) / 256)),
                     dim3(256), 0, stream, part, n, dsplit, C, B, out);
  return (int)hipGetLastError();
}
