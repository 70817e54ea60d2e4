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

// ---------------------------------------------------------------------------
// image_preprocess_k: crop / flip / bilinear resize / channel map / threshold /
// normalize / layout of a batch of images of any mix of sizes, in ONE launch.
// The contract (plan, arithmetic, limits) is in docs/kernels.md; the numpy
// reference is ops/cpu_ref.py::image_preprocess and gives the same bits.
//
// idesc: (n_img, 24) int64
//    0 src_off (elements)   1 Hs   2 Ws   3 Cs
//    4 pre_y0   5 pre_x0    6 Hc   7 Wc        pre-window of the source
//    8 flags: 1 pre flip x, 2 pre flip y, 4 post flip x, 8 post flip y,
//             16 resize (else copy path), 32 CHW output (else HWC)
//    9 Hr  10 Wr                                size after the resize
//   11 post_y0  12 post_x0  13 Ho  14 Wo       post-window of the resized
//   15 Co
//   16 channel map, one byte per output channel: 0..3 source channel, 4 gray
//   17 gray operands, one byte each: c0, c1, c2 (source channels)
//   18 out_off (elements)
//   19 n_ops   20 op kinds, one byte each (IMG_OP_*)
//   21..23 zero
// fdesc: (n_img, 34) float32
//    0 scale_y = (float)Hc / (float)Hr    1 scale_x = (float)Wc / (float)Wr
//    2 + 8 j ..: op j's operands: threshold {thr, maxVal, -}, normalize
//                {mean[0..3], std[0..3]}
// work_off: (n_img + 1) int64 prefix sum of image_work_items(Ho, Wo)
//
// A work item is a tile of 64 x 8 output pixels; the 256 threads are 64
// pixels wide x 4 rows, x fastest, and take two rows each.  Taps are read
// straight from the flat source (they are L2 hits: neighbouring pixels share
// them).  ops/backend.py::check_image_descriptors validates the descriptors
// before every launch; every index built from them is range-checked again
// here, so a bad descriptor reads zeros and writes nothing.
constexpr int IMG_TILE_W = 64;
constexpr int IMG_TILE_H = 8;
constexpr int IMG_DESC_I = 24;
constexpr int IMG_DESC_F = 34;

enum {
  IMG_OP_BINARY = 0,
  IMG_OP_BINARY_INV = 1,
  IMG_OP_TRUNC = 2,
  IMG_OP_TOZERO = 3,
  IMG_OP_TOZERO_INV = 4,
  IMG_OP_NORMALIZE = 5,
};

namespace {

struct ImgAxis {
  int i0, i1;
  float l0, l1;
};

// destination index d of an axis resized n_in -> n_out (scale = n_in / n_out)
__device__ inline ImgAxis img_axis(int d, float scale, int n_in) {
  float src = scale * ((float)d + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  ImgAxis a;
  a.i0 = max(0, min((int)floorf(src), n_in - 1));
  a.i1 = min(a.i0 + 1, n_in - 1);
  a.l1 = src - (float)a.i0;
  a.l0 = 1.0f - a.l1;
  return a;
}

__device__ inline float img_pick(const float (&s)[4], int c) {
  return c == 0 ? s[0] : (c == 1 ? s[1] : (c == 2 ? s[2] : s[3]));
}

__device__ inline void img_store(unsigned char* p, float v) {
  p[0] = (unsigned char)fminf(fmaxf(v, 0.f), 255.f);
}
__device__ inline void img_store(float* p, float v) { p[0] = v; }

}  // namespace

template <typename TS, typename TO>
__global__ __launch_bounds__(256) void image_preprocess_k(
    const TS* __restrict__ src, long src_numel,
    const long* __restrict__ idesc, const float* __restrict__ fdesc,
    const long* __restrict__ work_off, int n_img, TO* __restrict__ out,
    long out_numel) {
  // which image owns this tile: last i with work_off[i] <= item
  const long item = blockIdx.x;
  int lo = 0, hi = n_img;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (work_off[mid] <= item) lo = mid; else hi = mid;
  }
  const int img = lo;
  if (img < 0 || img >= n_img) return;
  const long* d = idesc + (long)IMG_DESC_I * img;
  const float* f = fdesc + (long)IMG_DESC_F * img;
  const long src_off = d[0];
  const int Hs = (int)d[1], Ws = (int)d[2], Cs = (int)d[3];
  const int pre_y0 = (int)d[4], pre_x0 = (int)d[5];
  const int Hc = (int)d[6], Wc = (int)d[7];
  const int flags = (int)d[8];
  const int post_y0 = (int)d[11], post_x0 = (int)d[12];
  const int Ho = (int)d[13], Wo = (int)d[14], Co = (int)d[15];
  const unsigned cmap = (unsigned)d[16], gmap = (unsigned)d[17];
  const long out_off = d[18];
  const int n_ops = min((int)d[19], 4);
  const unsigned kinds = (unsigned)d[20];
  const bool resize = flags & 16, chw = flags & 32;

  const int tiles_x = (Wo + IMG_TILE_W - 1) / IMG_TILE_W;
  const int local = (int)(item - work_off[img]);
  const int ox = (local % tiles_x) * IMG_TILE_W + (threadIdx.x & 63);
  const int oy_base = (local / tiles_x) * IMG_TILE_H + (threadIdx.x >> 6);
  if (ox >= Wo || Co < 1 || Co > 4 || Cs < 1 || Cs > 4) return;

  // x taps are the same for both rows of this thread
  const int rx = post_x0 + ((flags & 4) ? Wo - 1 - ox : ox);
  ImgAxis ax;
  if (resize) {
    ax = img_axis(rx, f[1], Wc);
  } else {
    ax.i0 = ax.i1 = rx; ax.l0 = 1.f; ax.l1 = 0.f;
  }
  const int sx0 = pre_x0 + ((flags & 1) ? Wc - 1 - ax.i0 : ax.i0);
  const int sx1 = pre_x0 + ((flags & 1) ? Wc - 1 - ax.i1 : ax.i1);
  const bool okx0 = sx0 >= 0 && sx0 < Ws, okx1 = sx1 >= 0 && sx1 < Ws;

#pragma unroll
  for (int rr = 0; rr < IMG_TILE_H / 4; ++rr) {
    const int oy = oy_base + 4 * rr;
    if (oy >= Ho) break;
    const int ry = post_y0 + ((flags & 8) ? Ho - 1 - oy : oy);
    ImgAxis ay;
    if (resize) {
      ay = img_axis(ry, f[0], Hc);
    } else {
      ay.i0 = ay.i1 = ry; ay.l0 = 1.f; ay.l1 = 0.f;
    }
    const int sy0 = pre_y0 + ((flags & 2) ? Hc - 1 - ay.i0 : ay.i0);
    const int sy1 = pre_y0 + ((flags & 2) ? Hc - 1 - ay.i1 : ay.i1);
    const bool oky0 = sy0 >= 0 && sy0 < Hs, oky1 = sy1 >= 0 && sy1 < Hs;
    const long b00 = src_off + ((long)sy0 * Ws + sx0) * Cs;
    const long b01 = src_off + ((long)sy0 * Ws + sx1) * Cs;
    const long b10 = src_off + ((long)sy1 * Ws + sx0) * Cs;
    const long b11 = src_off + ((long)sy1 * Ws + sx1) * Cs;
    const bool ok00 = oky0 && okx0 && b00 >= 0 && b00 + Cs <= src_numel;
    const bool ok01 = oky0 && okx1 && b01 >= 0 && b01 + Cs <= src_numel;
    const bool ok10 = oky1 && okx0 && b10 >= 0 && b10 + Cs <= src_numel;
    const bool ok11 = oky1 && okx1 && b11 >= 0 && b11 + Cs <= src_numel;

    // every source channel once
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= Cs) break;
      const float p00 = ok00 ? (float)src[b00 + c] : 0.f;
      if (resize) {
        const float p01 = ok01 ? (float)src[b01 + c] : 0.f;
        const float p10 = ok10 ? (float)src[b10 + c] : 0.f;
        const float p11 = ok11 ? (float)src[b11 + c] : 0.f;
        const float top = ax.l0 * p00 + ax.l1 * p01;
        const float bot = ax.l0 * p10 + ax.l1 * p11;
        s[c] = ay.l0 * top + ay.l1 * bot;
      } else {
        s[c] = p00;
      }
    }
    float gray = 0.f;
    if (((cmap | (cmap >> 8) | (cmap >> 16) | (cmap >> 24)) & 4) != 0) {
      const float c0 = img_pick(s, gmap & 3);
      const float c1 = img_pick(s, (gmap >> 8) & 3);
      const float c2 = img_pick(s, (gmap >> 16) & 3);
      gray = (0.299f * c2 + 0.587f * c1) + 0.114f * c0;
    }

#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= Co) break;
      const int code = (cmap >> (8 * k)) & 0xff;
      float v = code >= 4 ? gray : img_pick(s, code);
      for (int j = 0; j < n_ops; ++j) {
        const int kind = (kinds >> (8 * j)) & 0xff;
        const float* q = f + 2 + 8 * j;
        const float thr = q[0], mx = q[1];
        switch (kind) {
          case IMG_OP_BINARY: v = v > thr ? mx : 0.f; break;
          case IMG_OP_BINARY_INV: v = v > thr ? 0.f : mx; break;
          case IMG_OP_TRUNC: v = fminf(v, thr); break;
          case IMG_OP_TOZERO: v = v > thr ? v : 0.f; break;
          case IMG_OP_TOZERO_INV: v = v > thr ? 0.f : v; break;
          case IMG_OP_NORMALIZE: v = (v / 255.0f - q[k]) / q[4 + k]; break;
          default: break;
        }
      }
      const long o = chw ? out_off + ((long)k * Ho + oy) * Wo + ox
                         : out_off + ((long)oy * Wo + ox) * Co + k;
      if (o >= 0 && o < out_numel) img_store(out + o, v);
    }
  }
}

extern "C" long image_work_items(long Ho, long Wo) {
  if (Ho <= 0 || Wo <= 0) return 0;
  return ((Wo + IMG_TILE_W - 1) / IMG_TILE_W) *
         ((Ho + IMG_TILE_H - 1) / IMG_TILE_H);
}

// src_f32 / out_f32 select the element types (uint8 otherwise);
// n_items = work_off[n_img] is the grid size.
extern "C" void launch_image_preprocess(
    const void* src, long src_numel, int src_f32, const long* idesc,
    const float* fdesc, const long* work_off, int n_img, long n_items,
    void* out, long out_numel, int out_f32, hipStream_t stream) {
  if (n_img <= 0 || n_items <= 0) return;
  const dim3 grid((unsigned)n_items), block(256);
#define IMG_LAUNCH(TS, TO)                                                  \
  hipLaunchKernelGGL((image_preprocess_k<TS, TO>), grid, block, 0, stream,  \
                     (const TS*)src, src_numel, idesc, fdesc, work_off,     \
                     n_img, (TO*)out, out_numel)
  if (src_f32) {
    if (out_f32) IMG_LAUNCH(float, float);
    else IMG_LAUNCH(float, unsigned char);
  } else {
    if (out_f32) IMG_LAUNCH(unsigned char, float);
    else IMG_LAUNCH(unsigned char, unsigned char);
  }
#undef IMG_LAUNCH
}
