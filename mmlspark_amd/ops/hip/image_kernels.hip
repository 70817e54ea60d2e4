// Image-ingestion kernels for MI355X (gfx950, wave64).
//
// jpeg_reconstruct_k: everything a JPEG decoder does after entropy decoding —
// dequantisation, 8x8 IDCT, chroma replication, YCbCr->RGB and the crop from
// the MCU-padded planes — for a whole batch of images of mixed geometry in
// ONE launch.  The host (io_http/jpeg_parse.h) Huffman-decodes into int16
// coefficient planes; this kernel turns them into uint8 pixels on the device
// so the batch crosses PCIe as coefficients once and never as floats.
//
// The arithmetic is the host decoder's (io_http/jpeg_native.cpp), operation
// for operation, so the pixels are the host's:
//   dq[ZIGZAG[k]] = (double)coef[k] * q[k]
//   orthonormal separable IDCT in f64, terms added in order u = 0..7, v = 0..7
//   sample = (float)(px + 128.0)
//   chroma at (y / ry, x / rx), f32 colour formulas, (uint8)min(255,max(0,v+.5f))
// Contraction is switched off for the whole file: an fma rounds once where
// the host's mul + add round twice.
//
// Work decomposition: one 256-thread workgroup per work item.  An item is a
// horizontal run of G = max(1, 4 / (hmax*vmax)) MCUs, i.e. at most 32x32
// pixels and at most 48 blocks.  Each wave IDCTs one block at a time through
// LDS (lane = output sample, the row/column operands are LDS broadcasts) into
// per-component f32 planes in LDS; then all 256 threads convert pixels into
// an LDS byte stage, and the stage goes to global memory as whole dwords
// wherever the row's byte address allows (bytes only at a row's ragged ends).
// No atomics, no inter-workgroup communication: the output is a pure function
// of the input, bit-identical on every call.
//
// The descriptors are trusted here.  ops/backend.py::check_jpeg_descriptors
// validates them against the buffer sizes before every launch.
#include <hip/hip_runtime.h>

#include <cmath>

#pragma clang fp contract(off)

namespace {

struct IdctBasis {
  double b[64];  // b[x * 8 + u], orthonormal DCT-III
};

__device__ const unsigned char ZIGZAG_D[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ inline unsigned char to_u8(float v) {
  return (unsigned char)fminf(255.f, fmaxf(0.f, v + 0.5f));
}

}  // namespace

// coef:      (total_blocks, 64) int16, zigzag order
// qt:        (n_img, 4, 64) uint16, zigzag order
// img_desc:  (n_img, 4) int64  {W, H, nc, out_off}
// comp_desc: (n_img, 3, 4) int64  {h, v, tq, block_off}
// work_off:  (n_img + 1) int64 prefix sum of per-image work items
// out:       uint8, image i at out_off: H*W*3 (nc == 3) or H*W (nc == 1)
__global__ __launch_bounds__(256) void jpeg_reconstruct_k(
    const short* __restrict__ coef, const unsigned short* __restrict__ qt,
    const long* __restrict__ img_desc, const long* __restrict__ comp_desc,
    const long* __restrict__ work_off, int n_img, IdctBasis basis,
    unsigned char* __restrict__ out) {
  __shared__ double s_basis[64];
  __shared__ double s_dq[4][64];
  __shared__ double s_tmp[4][64];
  __shared__ float s_plane[3][32 * 32];
  __shared__ unsigned char s_rgb[32 * 96];

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  if (tid < 64) s_basis[tid] = basis.b[tid];

  // which image owns this work item: last i with work_off[i] <= item
  const long item = blockIdx.x;
  int lo = 0, hi = n_img;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (work_off[mid] <= item) lo = mid; else hi = mid;
  }
  const int img = lo;
  const long* d = img_desc + 4 * (long)img;
  const int W = (int)d[0], H = (int)d[1], nc = (int)d[2];
  const long out_off = d[3];
  const long* cd = comp_desc + 12 * (long)img;
  const int h0 = (int)cd[0], v0 = (int)cd[1], tq0 = (int)cd[2];
  const long bo0 = cd[3];
  int h1 = 1, v1 = 1, tq1 = 0, h2 = 1, v2 = 1, tq2 = 0;
  long bo1 = 0, bo2 = 0;
  if (nc == 3) {
    h1 = (int)cd[4]; v1 = (int)cd[5]; tq1 = (int)cd[6]; bo1 = cd[7];
    h2 = (int)cd[8]; v2 = (int)cd[9]; tq2 = (int)cd[10]; bo2 = cd[11];
  }
  // component 0 carries the maximal sampling factors (validated on the host)
  const int hmax = h0, vmax = v0;
  const int mcux = (W + 8 * hmax - 1) / (8 * hmax);
  const int G = (hmax * vmax >= 4) ? 1 : 4 / (hmax * vmax);
  const int items_x = (mcux + G - 1) / G;
  const int local = (int)(item - work_off[img]);
  const int my = local / items_x;
  const int mx0 = (local % items_x) * G;

  // ---- phase 1: dequantise + IDCT every block of the item into LDS planes
  const int n0 = h0 * G * v0;
  const int n1 = (nc == 3) ? h1 * G * v1 : 0;
  const int n2 = (nc == 3) ? h2 * G * v2 : 0;
  const int nblk = n0 + n1 + n2;
  const int y = lane >> 3, x = lane & 7;
  __syncthreads();
  for (int base = 0; base < nblk; base += 4) {
    const int t = base + wave;
    int c = 0, tt = t;
    if (t >= n0 + n1) { c = 2; tt = t - n0 - n1; }
    else if (t >= n0) { c = 1; tt = t - n0; }
    const int hc = c == 0 ? h0 : (c == 1 ? h1 : h2);
    const int vc = c == 0 ? v0 : (c == 1 ? v1 : v2);
    const int tqc = c == 0 ? tq0 : (c == 1 ? tq1 : tq2);
    const long boc = c == 0 ? bo0 : (c == 1 ? bo1 : bo2);
    const int cw = hc * G;            // blocks across in this item
    const int lby = tt / cw, lbx = tt % cw;
    const int bwc = mcux * hc;        // blocks across in the whole plane
    const int bx = mx0 * hc + lbx, by = my * vc + lby;
    // the last item of an MCU row may hold fewer than G MCUs
    const bool active = t < nblk && bx < bwc;
    if (active) {
      const long blk = boc + (long)by * bwc + bx;
      const double cv = (double)coef[blk * 64 + lane];
      const double q = (double)qt[((long)img * 4 + tqc) * 64 + lane];
      s_dq[wave][ZIGZAG_D[lane]] = cv * q;
    }
    __syncthreads();
    if (active) {
      double s = 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        s += s_basis[x * 8 + u] * s_dq[wave][y * 8 + u];
      s_tmp[wave][y * 8 + x] = s;
    }
    __syncthreads();
    if (active) {
      double s = 0.0;
#pragma unroll
      for (int v = 0; v < 8; ++v)
        s += s_basis[y * 8 + v] * s_tmp[wave][v * 8 + x];
      s_plane[c][(lby * 8 + y) * (cw * 8) + lbx * 8 + x] =
          (float)(s + 128.0);
    }
  }
  __syncthreads();

  // ---- phase 2: crop, replicate chroma, convert; bytes staged in LDS
  const int regW = 8 * hmax * G;
  const int X0 = mx0 * 8 * hmax, Y0 = my * 8 * vmax;
  const int cwid = min(regW, W - X0);
  const int chei = min(8 * vmax, H - Y0);
  const int bpp = (nc == 3) ? 3 : 1;
  const int rowbytes = cwid * bpp;
  if (nc == 3) {
    const int ryb = vmax / v1, rxb = hmax / h1, pwb = 8 * h1 * G;
    const int ryr = vmax / v2, rxr = hmax / h2, pwr = 8 * h2 * G;
    for (int p = tid; p < chei * cwid; p += 256) {
      const int py = p / cwid, px = p % cwid;
      const float Y = s_plane[0][py * regW + px];
      const float Cb = s_plane[1][(py / ryb) * pwb + px / rxb] - 128.f;
      const float Cr = s_plane[2][(py / ryr) * pwr + px / rxr] - 128.f;
      const float r = Y + 1.402f * Cr;
      const float g = Y - 0.344136f * Cb - 0.714136f * Cr;
      const float b = Y + 1.772f * Cb;
      unsigned char* o = s_rgb + py * rowbytes + px * 3;
      o[0] = to_u8(r);
      o[1] = to_u8(g);
      o[2] = to_u8(b);
    }
  } else {
    for (int p = tid; p < chei * cwid; p += 256) {
      const int py = p / cwid, px = p % cwid;
      s_rgb[py * rowbytes + px] = to_u8(s_plane[0][py * regW + px]);
    }
  }
  __syncthreads();

  // ---- phase 3: LDS stage -> global.  A row's bytes start at an arbitrary
  // address; slot s of a row is the aligned dword at (start & ~3) + 4 s.
  // Slots that lie wholly inside the row are one dword store, the ragged
  // first/last slots are byte stores (their other bytes belong to the
  // neighbouring work item).
  const int slots = rowbytes / 4 + 2;
  for (int t = tid; t < chei * slots; t += 256) {
    const int r = t / slots, s = t % slots;
    const long g = out_off + ((long)(Y0 + r) * W + X0) * bpp;
    const int first = s * 4 - (int)(g & 3);  // slot start, relative to g
    const int a = max(first, 0), b = min(first + 4, rowbytes);
    if (a >= b) continue;
    const unsigned char* src = s_rgb + r * rowbytes;
    if (b - a == 4) {
      const unsigned w = (unsigned)src[first] | ((unsigned)src[first + 1] << 8) |
                         ((unsigned)src[first + 2] << 16) |
                         ((unsigned)src[first + 3] << 24);
      *reinterpret_cast<unsigned*>(out + g + first) = w;
    } else {
      for (int i = a; i < b; ++i) out[g + i] = src[i];
    }
  }
}

// `out` must be 4-byte aligned; n_items = work_off[n_img] (the grid size).
extern "C" void launch_jpeg_reconstruct(
    const short* coef, const unsigned short* qt, const long* img_desc,
    const long* comp_desc, const long* work_off, int n_img, long n_items,
    unsigned char* out, hipStream_t stream) {
  if (n_img <= 0 || n_items <= 0) return;
  // the host decoder's basis, computed the way it computes it
  static const IdctBasis basis = [] {
    IdctBasis t;
    const double pi = 3.14159265358979323846;
    for (int x = 0; x < 8; ++x)
      for (int u = 0; u < 8; ++u) {
        const double a =
            (u == 0) ? std::sqrt(1.0 / 8.0) : std::sqrt(2.0 / 8.0);
        t.b[x * 8 + u] = a * std::cos((2 * x + 1) * u * pi / 16.0);
      }
    return t;
  }();
  hipLaunchKernelGGL(jpeg_reconstruct_k, dim3((unsigned)n_items), dim3(256), 0,
                     stream, coef, qt, img_desc, comp_desc, work_off, n_img,
                     basis, out);
}
