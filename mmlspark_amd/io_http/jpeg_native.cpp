// Native JPEG decoder — baseline (SOF0/SOF1) and progressive (SOF2).
//
// Replaces the pure-Python Huffman loop of io_http/jpeg_codec.py on the
// decode path (the round-1 image-ingestion bottleneck) with a C++
// implementation of ITU-T.81: canonical Huffman decode, spectral-selection
// and successive-approximation progressive scans (F.2 / G.2), restart
// markers, arbitrary sampling factors, orthonormal separable IDCT matching
// the Python codec's scipy idctn so both decoders agree to ±1 LSB.
// Completes the reference's ImageUtils decode surface
// (core/.../core/image/ImageUtils.scala) at native speed.
//
// The parser and entropy decoder live in jpeg_parse.h (no torch dependency,
// shared with tools/jpeg_parse_fuzz.cpp).  This file holds the two entry
// points: decode_jpeg reconstructs pixels on the host; decode_jpeg_coefficients
// stops after entropy decoding and exports the coefficient planes for the
// device reconstruction in ops/hip/image_kernels.hip.
#include <torch/extension.h>

#include "jpeg_parse.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

using namespace jpegparse;

namespace {

// orthonormal 8-point DCT-III basis (matches scipy idctn(norm="ortho"))
struct IdctBasis {
  double b[8][8];
  IdctBasis() {
    const double pi = 3.14159265358979323846;
    for (int x = 0; x < 8; ++x)
      for (int u = 0; u < 8; ++u) {
        double a = (u == 0) ? std::sqrt(1.0 / 8.0) : std::sqrt(2.0 / 8.0);
        b[x][u] = a * std::cos((2 * x + 1) * u * pi / 16.0);
      }
  }
};
const IdctBasis IDCT;

void idct8x8(const double* in, double* out) {
  double tmp[64];
  for (int y = 0; y < 8; ++y)      // rows: out(y,x) over u
    for (int x = 0; x < 8; ++x) {
      double s = 0;
      for (int u = 0; u < 8; ++u) s += IDCT.b[x][u] * in[y * 8 + u];
      tmp[y * 8 + x] = s;
    }
  for (int x = 0; x < 8; ++x)
    for (int y = 0; y < 8; ++y) {
      double s = 0;
      for (int v = 0; v < 8; ++v) s += IDCT.b[y][v] * tmp[v * 8 + x];
      out[y * 8 + x] = s;
    }
}

}  // namespace

torch::Tensor decode_jpeg_native(py::bytes data_b) {
  std::string s = data_b;  // copy; released during decode
  const uint8_t* data = (const uint8_t*)s.data();
  size_t n = s.size();
  py::gil_scoped_release nogil;

  Decoder dec(data, n);
  dec.parse();
  dec.check_reconstructible();

  const int W = dec.W, H = dec.H;
  const int nc = (int)dec.comps.size();
  // reconstruct each component plane at its own resolution
  std::vector<std::vector<float>> planes(nc);
  for (int ci = 0; ci < nc; ++ci) {
    Component& c = dec.comps[ci];
    const uint16_t* q = dec.qt[c.tq];
    planes[ci].assign((size_t)c.bh * 8 * c.bw * 8, 0.f);
    const int pw = c.bw * 8;
    double dq[64], px[64];
    for (int by = 0; by < c.bh; ++by)
      for (int bx = 0; bx < c.bw; ++bx) {
        const int32_t* blk = &c.coef[((size_t)by * c.bw + bx) * 64];
        for (int k = 0; k < 64; ++k) dq[ZIGZAG[k]] = (double)blk[k] * q[k];
        idct8x8(dq, px);
        float* dst = &planes[ci][(size_t)by * 8 * pw + bx * 8];
        for (int y = 0; y < 8; ++y)
          for (int x = 0; x < 8; ++x)
            dst[(size_t)y * pw + x] = (float)(px[y * 8 + x] + 128.0);
      }
  }

  torch::Tensor out;
  if (nc == 1) {
    out = torch::empty({H, W}, torch::kUInt8);
    uint8_t* o = out.data_ptr<uint8_t>();
    const int pw = dec.comps[0].bw * 8;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        float v = planes[0][(size_t)y * pw + x] + 0.5f;
        o[(size_t)y * W + x] =
            (uint8_t)std::min(255.f, std::max(0.f, v));
      }
  } else {
    out = torch::empty({H, W, 3}, torch::kUInt8);
    uint8_t* o = out.data_ptr<uint8_t>();
    const Component& cy = dec.comps[0];
    const Component& cb = dec.comps[1];
    const Component& cr = dec.comps[2];
    const int pwy = cy.bw * 8, pwb = cb.bw * 8, pwr = cr.bw * 8;
    const int ryb = dec.vmax / cb.v, rxb = dec.hmax / cb.h;
    const int ryr = dec.vmax / cr.v, rxr = dec.hmax / cr.h;
    for (int y = 0; y < H; ++y) {
      for (int x = 0; x < W; ++x) {
        float Y = planes[0][(size_t)y * pwy + x];
        float Cb = planes[1][(size_t)(y / ryb) * pwb + (x / rxb)] - 128.f;
        float Cr = planes[2][(size_t)(y / ryr) * pwr + (x / rxr)] - 128.f;
        float r = Y + 1.402f * Cr;
        float g = Y - 0.344136f * Cb - 0.714136f * Cr;
        float b = Y + 1.772f * Cb;
        uint8_t* px = o + ((size_t)y * W + x) * 3;
        px[0] = (uint8_t)std::min(255.f, std::max(0.f, r + 0.5f));
        px[1] = (uint8_t)std::min(255.f, std::max(0.f, g + 0.5f));
        px[2] = (uint8_t)std::min(255.f, std::max(0.f, b + 0.5f));
      }
    }
  }
  return out;
}

// Entropy decode only: the coefficient store in the layout the device
// reconstruction (ops/hip/image_kernels.hip) reads.  Returns
// (coef int16 (blocks, 64) zigzag, qt uint16 (4, 64) zigzag, W, H,
//  [(h, v, tq, bw, bh, block_off) per component]).
py::tuple decode_jpeg_coefficients(py::bytes data_b) {
  std::string s = data_b;
  Exported ex;
  torch::Tensor coef, qt;
  {
    py::gil_scoped_release nogil;
    Decoder dec((const uint8_t*)s.data(), s.size());
    dec.parse();
    export_coefficients(dec, ex);
    coef = torch::empty({(int64_t)ex.blocks, 64}, torch::kInt16);
    std::memcpy(coef.data_ptr<int16_t>(), ex.coef.data(),
                ex.coef.size() * sizeof(int16_t));
    qt = torch::empty({4, 64}, torch::kUInt16);
    std::memcpy(qt.data_ptr(), ex.qt, sizeof(ex.qt));
  }
  py::list comps;
  for (int ci = 0; ci < ex.nc; ++ci) {
    const CompGeom& g = ex.comp[ci];
    comps.append(py::make_tuple(g.h, g.v, g.tq, g.bw, g.bh, g.block_off));
  }
  return py::make_tuple(coef, qt, ex.W, ex.H, comps);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("decode_jpeg", &decode_jpeg_native,
        "native JPEG decode (baseline + progressive) -> uint8 HxW[x3]");
  m.def("decode_jpeg_coefficients", &decode_jpeg_coefficients,
        "entropy decode only -> (coef int16, qt uint16, W, H, components)");
}
