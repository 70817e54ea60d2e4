// Superpixel kernels for the image explainers on MI355X (gfx950, wave64).
//
// slic_assign_k + slic_update_k: the k-means of explainers/sampler.py::
// slic_superpixels over a whole column of uint8 images of any mix of sizes,
// two launches per iteration for the column.  masked_image_batch_k: every
// perturbed sample of one image, written straight into the model's float32
// NCHW input batch.  The contract of both is ops/cpu_ref.py::slic_segment and
// ::masked_image_batch.
//
// SLIC.  A pixel has five float32 features, [r, g, b] / modifier, y / cell,
// x / cell, each one correctly rounded divide as numpy does it.  A work item
// is a run of SLIC_TILE = 1024 consecutive pixels of one image (row-major, so
// a tile is a few rows or a piece of one); a descriptor table and a prefix sum
// of the images' tile counts map blockIdx.x to (image, tile), as
// image_preprocess_k does.  The 256 lanes hold four pixels each (tile offset
// j * 256 + lane, so loads and the label stores are coalesced): the five
// features and the running (best distance, best index) of every pixel stay in
// registers.  The image's centres are staged in LDS SLIC_CHUNK = 1024 at a
// time, eight floats apart so one centre is two 16-byte reads, and every lane
// sweeps the chunk reading the same address (an LDS broadcast, no bank
// conflict).  The distance is the direct sum ((((dr^2 + dg^2) + db^2) + dy^2)
// + dx^2), each square rounded before it is added (contraction is off for the
// whole file); it is never expanded into |p|^2 - 2 p.c + |c|^2, which rounds
// differently near ties.  `<` keeps the lowest index among equal distances.
// The inner dimension is 5: vector FP32 work, nothing for MFMA.
//
// The mean update is exact.  Pixels are uint8 and coordinates are integers, so
// a cluster's sums of r, g, b, y, x and its count are integers.  After the
// sweep a block goes over the centre chunks once more; for every chunk that
// one of its pixels chose (__syncthreads_or) it clears 6 x 1024 uint32 cells
// in LDS, adds its pixels with LDS integer atomics and flushes the touched
// cells with 64-bit integer atomics to the global (K, 6) table.  The sums do
// not depend on the order of the adds.  A block adds at most 1024 pixels to a
// 32-bit cell, each at most max(255, H - 1, W - 1); with H, W <= SLIC_MAX_DIM
// = 32768 that stays below 2^25.  The launcher checks that limit, and
// H * W < 2^31 so that a pixel index is an int.
//
// The centres are recomputed by a tiny kernel of their own, slic_update_k,
// one thread per centre, rather than while the next assignment stages its LDS
// copy: the binding returns the updated centres after the last iteration
// anyway, every block of the next sweep would otherwise repeat the same K
// 64-bit divides, and the kernel also clears the sum cells for the next
// iteration (no memset between launches).  centre = (double)sum / (double)count
// / scale, rounded to float once; an empty cluster keeps its centre bit for bit.
//
// masked_image_batch_k.  A block owns 256 consecutive output pixels of the
// size x size plane.  Each lane computes, once, what all samples share: the
// bilinear tap geometry of torch's align_corners=False resize (one tap when
// the image already has the output size), the up to four source values per
// channel already mapped through the k / 255 table, and for every tap the
// word and bit of its own pixel's segment.  Then the block loops over its
// share of the samples; the samples' bit-packed state rows are staged in LDS
// in chunks of 8192 words, a lane tests its taps' bits (neighbouring lanes
// share segments, so most reads are broadcasts), replaces the taps whose
// segment is off by the fill and blends.  The source and the segment map are
// read once per block, not once per sample, so the traffic is the output
// stream: three coalesced float stores per lane and sample.  gridDim.y splits
// the samples so that small planes still fill the device.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

constexpr int SLIC_THREADS = 256;
constexpr int SLIC_PPT = 4;                         // pixels per lane
constexpr int SLIC_TILE = SLIC_THREADS * SLIC_PPT;  // pixels per work item
constexpr int SLIC_CHUNK = 1024;                    // centres staged at a time
constexpr int SLIC_MAX_K = 4096;
constexpr int SLIC_MAX_DIM = 32768;
constexpr int SLIC_DESC = 8;
constexpr int MASK_THREADS = 256;
constexpr int MASK_LDS_WORDS = 8192;
constexpr int MASK_MAX_SEGMENTS = 4096;

// idesc: (n_img, 8) int64
//   0 src_off (bytes into src)  1 H  2 W  3 C (1 or 3)  4 K
//   5 ctr_off (rows of centres / sums)  6 lab_off (pixels into labels)
//   7 cell (the image's cell size; images of one column may differ in it)
// work_off: (n_img + 1) int64 prefix sum of ceil(H * W / 1024)

namespace {

__device__ inline int slic_image_of(const long* __restrict__ work_off,
                                    int n_img, long item) {
  int lo = 0, hi = n_img;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (work_off[mid] <= item) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace

// Default seeding: centre k sits on the pixel (cell/2 + (k / gw) * cell,
// cell/2 + (k % gw) * cell) and takes its features.
__global__ __launch_bounds__(SLIC_THREADS) void slic_seed_k(
    const unsigned char* __restrict__ src, long src_numel,
    const long* __restrict__ idesc, float* __restrict__ centres, long total_k,
    float mod) {
  const long* d = idesc + (long)SLIC_DESC * blockIdx.y;
  const int W = (int)d[2], C = (int)d[3], K = (int)d[4], cell = (int)d[7];
  const int k = blockIdx.x * SLIC_THREADS + threadIdx.x;
  if (k >= K || cell < 1 || W <= cell / 2 || d[5] + k >= total_k) return;
  const int gw = (W - cell / 2 + cell - 1) / cell;  // centres per grid row
  const int y = cell / 2 + (k / gw) * cell, x = cell / 2 + (k % gw) * cell;
  const long b = d[0] + ((long)y * W + x) * C;
  if (b < 0 || b + C > src_numel) return;
  const float fc = (float)cell;
  float* c = centres + (d[5] + k) * 5;
  c[0] = (float)src[b] / mod;
  c[1] = (float)src[b + (C == 3 ? 1 : 0)] / mod;
  c[2] = (float)src[b + (C == 3 ? 2 : 0)] / mod;
  c[3] = (float)y / fc;
  c[4] = (float)x / fc;
}

__global__ __launch_bounds__(SLIC_THREADS) void slic_assign_k(
    const unsigned char* __restrict__ src, long src_numel,
    const long* __restrict__ idesc, const long* __restrict__ work_off,
    int n_img, const float* __restrict__ centres, long total_k,
    unsigned long long* __restrict__ sums, int* __restrict__ labels,
    long lab_numel, float mod) {
  // the sums (6 words a cluster) reuse the centres' LDS (8 words a centre):
  // the sweep is over, and a barrier stands between the two uses
  __shared__ float4 s_c[SLIC_CHUNK * 2];
  unsigned* s_sum = reinterpret_cast<unsigned*>(s_c);

  const int tid = threadIdx.x;
  const long item = blockIdx.x;
  const int img = slic_image_of(work_off, n_img, item);
  const long* d = idesc + (long)SLIC_DESC * img;
  const long src_off = d[0];
  const int H = (int)d[1], W = (int)d[2], C = (int)d[3];
  const long ctr_off = d[5], lab_off = d[6];
  const float cell = (float)d[7];
  const int npix = H * W;
  // never past the tables, whatever the descriptor says
  const int K = (int)min((long)min((int)d[4], SLIC_MAX_K), total_k - ctr_off);
  const int p0 = (int)(item - work_off[img]) * SLIC_TILE + tid;

  float f[SLIC_PPT][5], best[SLIC_PPT];
  int bi[SLIC_PPT], py[SLIC_PPT], px[SLIC_PPT];
  unsigned rgb[SLIC_PPT];
  bool ok[SLIC_PPT];
#pragma unroll
  for (int j = 0; j < SLIC_PPT; ++j) {
    const int p = p0 + j * SLIC_THREADS;
    const long b = src_off + (long)p * C;
    ok[j] = p < npix && b >= 0 && b + C <= src_numel &&
            lab_off + p < lab_numel;
    py[j] = ok[j] ? p / W : 0;
    px[j] = ok[j] ? p - py[j] * W : 0;
    unsigned r = 0, g = 0, bl = 0;
    if (ok[j]) {
      r = src[b];
      g = C == 3 ? src[b + 1] : r;
      bl = C == 3 ? src[b + 2] : r;
    }
    rgb[j] = r | (g << 8) | (bl << 16);
    f[j][0] = (float)r / mod;
    f[j][1] = (float)g / mod;
    f[j][2] = (float)bl / mod;
    f[j][3] = (float)py[j] / cell;
    f[j][4] = (float)px[j] / cell;
    best[j] = INFINITY;
    bi[j] = 0;
  }

  // ---- sweep every centre of the image, a chunk in LDS at a time
  for (int k0 = 0; k0 < K; k0 += SLIC_CHUNK) {
    const int n = min(SLIC_CHUNK, K - k0);
    __syncthreads();
    for (int i = tid; i < n; i += SLIC_THREADS) {
      const float* c = centres + (ctr_off + k0 + i) * 5;
      s_c[2 * i] = make_float4(c[0], c[1], c[2], c[3]);
      s_c[2 * i + 1] = make_float4(c[4], 0.f, 0.f, 0.f);
    }
    __syncthreads();
    for (int c = 0; c < n; ++c) {
      const float4 a = s_c[2 * c];
      const float c4 = s_c[2 * c + 1].x;
#pragma unroll
      for (int j = 0; j < SLIC_PPT; ++j) {
        const float d0 = f[j][0] - a.x, d1 = f[j][1] - a.y;
        const float d2 = f[j][2] - a.z, d3 = f[j][3] - a.w;
        const float d4 = f[j][4] - c4;
        const float dist =
            (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3) + d4 * d4;
        if (dist < best[j]) {
          best[j] = dist;
          bi[j] = k0 + c;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < SLIC_PPT; ++j)
    if (ok[j]) labels[lab_off + p0 + j * SLIC_THREADS] = bi[j];

  // ---- exact per-cluster sums: LDS integer atomics, one flush per chunk
  for (int k0 = 0; k0 < K; k0 += SLIC_CHUNK) {
    const int n = min(SLIC_CHUNK, K - k0);
    int hit = 0;
#pragma unroll
    for (int j = 0; j < SLIC_PPT; ++j)
      hit |= ok[j] && bi[j] >= k0 && bi[j] < k0 + n;
    if (!__syncthreads_or(hit)) continue;
    for (int i = tid; i < n * 6; i += SLIC_THREADS) s_sum[i] = 0u;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SLIC_PPT; ++j) {
      if (!(ok[j] && bi[j] >= k0 && bi[j] < k0 + n)) continue;
      unsigned* s = s_sum + (bi[j] - k0) * 6;
      atomicAdd(s + 0, rgb[j] & 255u);
      atomicAdd(s + 1, (rgb[j] >> 8) & 255u);
      atomicAdd(s + 2, rgb[j] >> 16);
      atomicAdd(s + 3, (unsigned)py[j]);
      atomicAdd(s + 4, (unsigned)px[j]);
      atomicAdd(s + 5, 1u);
    }
    __syncthreads();
    for (int i = tid; i < n; i += SLIC_THREADS) {
      if (s_sum[i * 6 + 5] == 0u) continue;
      unsigned long long* g = sums + (ctr_off + k0 + i) * 6;
#pragma unroll
      for (int q = 0; q < 6; ++q)
        atomicAdd(g + q, (unsigned long long)s_sum[i * 6 + q]);
    }
  }
}

__global__ __launch_bounds__(SLIC_THREADS) void slic_update_k(
    const long* __restrict__ idesc, float* __restrict__ centres,
    unsigned long long* __restrict__ sums, long total_k, float mod) {
  const long* d = idesc + (long)SLIC_DESC * blockIdx.y;
  const int K = (int)d[4];
  const float cell = (float)d[7];
  const int k = blockIdx.x * SLIC_THREADS + threadIdx.x;
  if (k >= K || d[5] + k >= total_k) return;
  unsigned long long* s = sums + (d[5] + k) * 6;
  const unsigned long long cnt = s[5];
  if (cnt == 0ull) return;          // nothing to clear, the centre stays
  float* c = centres + (d[5] + k) * 5;
  const double n = (double)cnt;
#pragma unroll
  for (int q = 0; q < 5; ++q)
    c[q] = (float)((double)s[q] / n / (double)(q < 3 ? mod : cell));
#pragma unroll
  for (int q = 0; q < 6; ++q) s[q] = 0ull;
}

// Runs n_iter iterations over the column.  `sums` must be zero on entry and
// is zero again on return.  seed != 0 fills `centres` from the grid first.
extern "C" int launch_slic_segment(
    const unsigned char* src, long src_numel, const long* idesc,
    const long* work_off, int n_img, long n_items, int max_k, long total_k,
    float* centres, unsigned long long* sums, int* labels, long lab_numel,
    float mod, int n_iter, int seed, hipStream_t stream) {
  if (n_img <= 0 || n_items <= 0 || max_k <= 0) return 0;
  if (max_k > SLIC_MAX_K || n_items >= (1L << 31)) return -1;
  const dim3 per_centre((max_k + SLIC_THREADS - 1) / SLIC_THREADS, n_img);
  if (seed)
    hipLaunchKernelGGL(slic_seed_k, per_centre, dim3(SLIC_THREADS), 0, stream,
                       src, src_numel, idesc, centres, total_k, mod);
  for (int it = 0; it < n_iter; ++it) {
    hipLaunchKernelGGL(slic_assign_k, dim3((unsigned)n_items),
                       dim3(SLIC_THREADS), 0, stream, src, src_numel, idesc,
                       work_off, n_img, centres, total_k, sums, labels,
                       lab_numel, mod);
    hipLaunchKernelGGL(slic_update_k, per_centre, dim3(SLIC_THREADS), 0,
                       stream, idesc, centres, sums, total_k, mod);
  }
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
namespace {

struct MaskAxis {
  int i0, i1;
  float l0, l1;
};

// torch's align_corners=False source index of destination d; scale = in / out
__device__ inline MaskAxis mask_axis(int d, float scale, int n_in) {
  float s = scale * ((float)d + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  MaskAxis a;
  a.i0 = min((int)s, n_in - 1);
  a.i1 = min(a.i0 + 1, n_in - 1);
  a.l1 = s - (float)a.i0;
  a.l0 = 1.0f - a.l1;
  return a;
}

}  // namespace

// img (H, W, C) uint8, seg (H, W) int32, states (n, words) bit rows, lut (256)
// -> out (n, 3, size, size) float32.  A segment outside [0, m) is never off.
__global__ __launch_bounds__(MASK_THREADS) void masked_image_batch_k(
    const unsigned char* __restrict__ img, int H, int W, int C,
    const int* __restrict__ seg, const unsigned* __restrict__ states,
    int n_samples, int words, int m, int fill, int size, float sy, float sx,
    const float* __restrict__ lut, float* __restrict__ out, int per_split) {
  __shared__ unsigned s_st[MASK_LDS_WORDS];
  __shared__ float s_lut[256];
  const int tid = threadIdx.x;
  s_lut[tid] = lut[tid];
  __syncthreads();

  const int plane = size * size;
  const int pix = blockIdx.x * MASK_THREADS + tid;
  const bool valid = pix < plane;
  const bool resize = H != size || W != size;
  const int oy = valid ? pix / size : 0, ox = valid ? pix - oy * size : 0;
  MaskAxis ay, ax;
  if (resize) {
    ay = mask_axis(oy, sy, H);
    ax = mask_axis(ox, sx, W);
  } else {
    ay.i0 = ay.i1 = oy; ay.l0 = 1.f; ay.l1 = 0.f;
    ax.i0 = ax.i1 = ox; ax.l0 = 1.f; ax.l1 = 0.f;
  }
  // the taps, read once for all samples: 00, 01, 10, 11
  float v[4][3];
  int wi[4];
  unsigned bm[4], always[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int y = (t & 2) ? ay.i1 : ay.i0, x = (t & 1) ? ax.i1 : ax.i0;
    const long p = (long)y * W + x;
    const int sg = seg[p];
    const bool in = sg >= 0 && sg < m;
    wi[t] = in ? sg >> 5 : 0;
    bm[t] = in ? 1u << (sg & 31) : 0u;
    always[t] = in ? 0u : 1u;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      v[t][c] = s_lut[img[p * C + (C == 3 ? c : 0)]];
  }
  const float fv = s_lut[fill & 255];

  const int s_begin = blockIdx.y * per_split;
  const int s_end = min(n_samples, s_begin + per_split);
  const int rows_per = MASK_LDS_WORDS / words;
  for (int s0 = s_begin; s0 < s_end; s0 += rows_per) {
    const int rows = min(rows_per, s_end - s0);
    __syncthreads();
    for (int i = tid; i < rows * words; i += MASK_THREADS)
      s_st[i] = states[(long)s0 * words + i];
    __syncthreads();
    if (!valid) continue;
    for (int r = 0; r < rows; ++r) {
      const unsigned* row = s_st + r * words;
      float* o = out + (long)(s0 + r) * 3 * plane + pix;
      const bool on0 = (row[wi[0]] & bm[0]) | always[0];
      if (!resize) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[(long)c * plane] = on0 ? v[0][c] : fv;
        continue;
      }
      const bool on1 = (row[wi[1]] & bm[1]) | always[1];
      const bool on2 = (row[wi[2]] & bm[2]) | always[2];
      const bool on3 = (row[wi[3]] & bm[3]) | always[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float p00 = on0 ? v[0][c] : fv, p01 = on1 ? v[1][c] : fv;
        const float p10 = on2 ? v[2][c] : fv, p11 = on3 ? v[3][c] : fv;
        const float top = ax.l0 * p00 + ax.l1 * p01;
        const float bot = ax.l0 * p10 + ax.l1 * p11;
        o[(long)c * plane] = ay.l0 * top + ay.l1 * bot;
      }
    }
  }
}

extern "C" int launch_masked_image_batch(
    const unsigned char* img, int H, int W, int C, const int* seg,
    const unsigned* states, int n_samples, int words, int m, int fill,
    int size, const float* lut, float* out, hipStream_t stream) {
  if (n_samples <= 0) return 0;
  if (H < 1 || W < 1 || (C != 1 && C != 3) || size < 1 ||
      size > SLIC_MAX_DIM || m < 1 || m > MASK_MAX_SEGMENTS ||
      words != (m + 31) / 32)
    return -1;
  const long plane = (long)size * size;
  if (plane >= (1L << 31)) return -1;
  const int tiles = (int)((plane + MASK_THREADS - 1) / MASK_THREADS);
  // enough blocks for a few waves per CU; a split keeps at least 32 samples
  int splits = (2048 + tiles - 1) / tiles;
  splits = max(1, min(splits, (n_samples + 31) / 32));
  const int per_split = (n_samples + splits - 1) / splits;
  splits = (n_samples + per_split - 1) / per_split;
  hipLaunchKernelGGL(masked_image_batch_k, dim3(tiles, splits),
                     dim3(MASK_THREADS), 0, stream, img, H, W, C, seg, states,
                     n_samples, words, m, fill, size,
                     (float)H / (float)size, (float)W / (float)size, lut, out,
                     per_split);
  return (int)hipGetLastError();
}
