// JPEG parser + entropy decoder — baseline (SOF0/SOF1) and progressive (SOF2).
//
// Header-only, no torch / pybind dependency: shared by jpeg_native.cpp (the
// Python extension) and tools/jpeg_parse_fuzz.cpp (a stand-alone sanitizer
// harness).  Implements ITU-T.81 canonical Huffman decode, spectral-selection
// and successive-approximation progressive scans (F.2 / G.2), restart
// markers and arbitrary sampling factors.  Both scan types end in the
// per-component coefficient store Component::coef; reconstruction (dequant,
// IDCT, colour) lives with the callers — on the host in jpeg_native.cpp, on
// the GPU in ops/hip/image_kernels.hip, fed by export_coefficients() below.
//
// Every length, table id and index read from the stream is checked before
// it is used; a malformed stream throws std::runtime_error.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

namespace jpegparse {

// largest frame the decoders accept (W*H samples per full-size plane)
constexpr int64_t MAX_PIXELS = int64_t(1) << 26;

struct HuffTable {
  // canonical decode tables (F.2.2.3)
  int32_t mincode[17] = {};
  int32_t maxcode[18] = {};
  int32_t valptr[17] = {};
  uint8_t vals[256] = {};
  bool present = false;

  void build(const uint8_t* bits, const uint8_t* values, int nvals) {
    if (nvals < 0 || nvals > 256)
      throw std::runtime_error("huffman table with more than 256 symbols");
    std::memcpy(vals, values, nvals);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
      valptr[l] = k;
      mincode[l] = code;
      code += bits[l - 1];
      k += bits[l - 1];
      maxcode[l] = code - 1;
      if (bits[l - 1] == 0) maxcode[l] = -1;
      code <<= 1;
    }
    maxcode[17] = 0x7fffffff;
    present = true;
  }
};

struct BitReader {
  const uint8_t* data;
  size_t n;
  size_t pos = 0;
  uint32_t bitbuf = 0;
  int bitcnt = 0;
  bool hit_marker = false;  // stopped at a non-RST marker

  BitReader(const uint8_t* d, size_t len) : data(d), n(len) {}

  int next_byte() {
    // returns -1 at a non-RST marker (end of entropy data)
    while (pos < n) {
      uint8_t b = data[pos];
      if (b != 0xFF) { ++pos; return b; }
      if (pos + 1 >= n) { hit_marker = true; return -1; }
      uint8_t m = data[pos + 1];
      if (m == 0x00) { pos += 2; return 0xFF; }
      if (m >= 0xD0 && m <= 0xD7) { hit_marker = true; return -1; }
      hit_marker = true;
      return -1;  // real marker: stop (pos stays at the 0xFF)
    }
    hit_marker = true;
    return -1;
  }

  int read_bit() {
    if (bitcnt == 0) {
      int b = next_byte();
      if (b < 0) return 0;  // pad with 0s past the marker (spec behaviour)
      bitbuf = (uint32_t)b;
      bitcnt = 8;
    }
    bitcnt--;
    return (bitbuf >> bitcnt) & 1;
  }

  int read_bits(int nb) {
    int v = 0;
    for (int i = 0; i < nb; ++i) v = (v << 1) | read_bit();
    return v;
  }

  void align_and_skip_rst() {
    bitcnt = 0;
    // skip to and over the RSTn marker
    while (pos + 1 < n) {
      if (data[pos] == 0xFF && data[pos + 1] >= 0xD0 &&
          data[pos + 1] <= 0xD7) {
        pos += 2;
        hit_marker = false;
        return;
      }
      ++pos;
    }
  }
};

inline int extend(int v, int t) {
  return (t && v < (1 << (t - 1))) ? v - (1 << t) + 1 : v;
}

inline int decode_huff(BitReader& br, const HuffTable& h) {
  int code = br.read_bit();
  int l = 1;
  while (code > h.maxcode[l]) {
    code = (code << 1) | br.read_bit();
    if (++l > 16) throw std::runtime_error("bad huffman code");
  }
  // an over-subscribed (invalid) table can put the index outside vals[]
  const int idx = h.valptr[l] + code - h.mincode[l];
  if (idx < 0 || idx > 255) throw std::runtime_error("bad huffman code");
  return h.vals[idx];
}

// two's-complement helpers: a hostile stream can drive the DC predictor and
// the successive-approximation shifts past int range; wrap instead of
// overflowing (valid streams never get near it)
inline int wrap_add(int a, int b) { return (int)((uint32_t)a + (uint32_t)b); }
inline int32_t wrap_shl(int v, int s) {
  return (int32_t)((uint32_t)v << s);
}

struct Component {
  int id = 0, h = 1, v = 1, tq = 0;
  int td = 0, ta = 0;       // current scan's tables
  int bw = 0, bh = 0;        // blocks across / down (full, MCU padded)
  std::vector<int32_t> coef; // bw*bh blocks × 64, zigzag order
};

static const int ZIGZAG[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Decoder {
  const uint8_t* data;
  size_t n;
  size_t pos = 2;
  int W = 0, H = 0;
  int precision = 8;
  bool progressive = false;
  int hmax = 1, vmax = 1, mcux = 0, mcuy = 0;
  std::vector<Component> comps;
  uint16_t qt[4][64] = {};
  HuffTable dc[4], ac[4];
  int dri = 0;
  int eobrun = 0;

  explicit Decoder(const uint8_t* d, size_t len) : data(d), n(len) {}

  uint16_t u16(size_t p) const { return (data[p] << 8) | data[p + 1]; }

  void parse() {
    if (n < 4 || data[0] != 0xFF || data[1] != 0xD8)
      throw std::runtime_error("not a JPEG");
    bool got_frame = false;
    while (pos + 4 <= n) {
      if (data[pos] != 0xFF) { ++pos; continue; }
      uint8_t m = data[pos + 1];
      if (m == 0xFF) { ++pos; continue; }  // fill byte before a marker
      pos += 2;
      if (m == 0xD8 || m == 0x01 || m == 0x00 || (m >= 0xD0 && m <= 0xD7))
        continue;
      if (m == 0xD9) break;  // EOI
      size_t seglen = u16(pos);
      if (seglen < 2 || pos + seglen > n)
        throw std::runtime_error("segment length runs past the stream");
      size_t segend = pos + seglen;
      const uint8_t* seg = data + pos + 2;
      size_t sn = seglen - 2;
      if (m == 0xDB) {
        size_t o = 0;
        while (o < sn) {
          int pq = seg[o] >> 4, tq2 = seg[o] & 15;
          ++o;
          if (pq > 1 || tq2 > 3)
            throw std::runtime_error("bad quantisation table id");
          if (o + (pq ? 128 : 64) > sn)
            throw std::runtime_error("truncated DQT segment");
          for (int k = 0; k < 64; ++k) {
            if (pq) { qt[tq2][k] = (seg[o] << 8) | seg[o + 1]; o += 2; }
            else qt[tq2][k] = seg[o + k];
          }
          if (!pq) o += 64;
        }
      } else if (m == 0xC4) {
        size_t o = 0;
        while (o + 17 <= sn) {
          int tc = seg[o] >> 4, th = seg[o] & 15;
          if (tc > 1 || th > 3)
            throw std::runtime_error("bad huffman table id");
          const uint8_t* bits = seg + o + 1;
          int nv = 0;
          for (int i = 0; i < 16; ++i) nv += bits[i];
          if (nv > 256 || o + 17 + (size_t)nv > sn)
            throw std::runtime_error("bad huffman table size");
          (tc ? ac[th] : dc[th]).build(bits, seg + o + 17, nv);
          o += 17 + nv;
        }
      } else if (m == 0xC0 || m == 0xC1 || m == 0xC2) {
        if (sn < 6) throw std::runtime_error("truncated SOF segment");
        progressive = (m == 0xC2);
        precision = seg[0];
        H = (seg[1] << 8) | seg[2];
        W = (seg[3] << 8) | seg[4];
        int nc = seg[5];
        if (sn < 6 + 3 * (size_t)nc)
          throw std::runtime_error("truncated SOF segment");
        if (W < 1 || H < 1 || (int64_t)W * H > MAX_PIXELS)
          throw std::runtime_error("unsupported frame size");
        if (nc > 4) throw std::runtime_error("unsupported component count");
        comps.assign(nc, Component());
        for (int i = 0; i < nc; ++i) {
          comps[i].id = seg[6 + 3 * i];
          comps[i].h = seg[7 + 3 * i] >> 4;
          comps[i].v = seg[7 + 3 * i] & 15;
          comps[i].tq = seg[8 + 3 * i];
          if (comps[i].h < 1 || comps[i].h > 4 || comps[i].v < 1 ||
              comps[i].v > 4)
            throw std::runtime_error("bad sampling factor");
          if (comps[i].tq > 3)
            throw std::runtime_error("bad quantisation table id");
        }
        hmax = vmax = 1;
        for (auto& c : comps) { hmax = std::max(hmax, c.h);
                                vmax = std::max(vmax, c.v); }
        mcux = (W + 8 * hmax - 1) / (8 * hmax);
        mcuy = (H + 8 * vmax - 1) / (8 * vmax);
        for (auto& c : comps) {
          c.bw = mcux * c.h;
          c.bh = mcuy * c.v;
          c.coef.assign((size_t)c.bw * c.bh * 64, 0);
        }
        got_frame = true;
      } else if (m == 0xC3 || (m >= 0xC5 && m <= 0xCF && m != 0xC8)) {
        throw std::runtime_error("unsupported SOF marker");
      } else if (m == 0xDD) {
        if (sn < 2) throw std::runtime_error("truncated DRI segment");
        dri = (seg[0] << 8) | seg[1];
      } else if (m == 0xDA) {
        if (!got_frame) throw std::runtime_error("SOS before SOF");
        if (sn < 1) throw std::runtime_error("truncated SOS segment");
        int ns = seg[0];
        if (sn < 4 + 2 * (size_t)ns)
          throw std::runtime_error("truncated SOS segment");
        std::vector<int> sel;
        for (int i = 0; i < ns; ++i) {
          int cs = seg[1 + 2 * i], tda = seg[2 + 2 * i];
          if ((tda >> 4) > 3 || (tda & 15) > 3)
            throw std::runtime_error("bad huffman table id");
          for (size_t ci = 0; ci < comps.size(); ++ci)
            if (comps[ci].id == cs) {
              comps[ci].td = tda >> 4;
              comps[ci].ta = tda & 15;
              sel.push_back((int)ci);
            }
        }
        if (sel.empty())
          throw std::runtime_error("scan selects no frame component");
        int Ss = seg[1 + 2 * ns], Se = seg[2 + 2 * ns];
        int Ah = seg[3 + 2 * ns] >> 4, Al = seg[3 + 2 * ns] & 15;
        if (Ss > Se || Se > 63 || Al > 13)
          throw std::runtime_error("bad scan parameters");
        pos = segend;
        decode_scan(sel, Ss, Se, Ah, Al);
        continue;  // pos updated past the entropy data
      }
      pos = segend;
    }
  }

  void decode_scan(const std::vector<int>& sel, int Ss, int Se, int Ah,
                   int Al) {
    BitReader br(data, n);
    br.pos = pos;
    eobrun = 0;
    std::vector<int> pred(comps.size(), 0);

    const bool interleaved = sel.size() > 1;
    long unit_count = 0;
    auto maybe_rst = [&]() {
      if (dri && unit_count && unit_count % dri == 0) {
        br.align_and_skip_rst();
        std::fill(pred.begin(), pred.end(), 0);
        eobrun = 0;
      }
    };

    if (interleaved || (!progressive && sel.size() == comps.size() &&
                        comps.size() > 1)) {
      for (int my = 0; my < mcuy; ++my)
        for (int mx = 0; mx < mcux; ++mx) {
          maybe_rst();
          for (int ci : sel) {
            Component& c = comps[ci];
            for (int vy = 0; vy < c.v; ++vy)
              for (int vx = 0; vx < c.h; ++vx) {
                int bx = mx * c.h + vx, by = my * c.v + vy;
                int32_t* blk = &c.coef[((size_t)by * c.bw + bx) * 64];
                decode_block(br, c, blk, pred[ci], Ss, Se, Ah, Al);
              }
          }
          ++unit_count;
        }
    } else {
      // non-interleaved: one component, block raster over ITS OWN grid
      int ci = sel[0];
      Component& c = comps[ci];
      int bw = (W * c.h + 8 * hmax - 1) / (8 * hmax);
      int bh = (H * c.v + 8 * vmax - 1) / (8 * vmax);
      for (int by = 0; by < bh; ++by)
        for (int bx = 0; bx < bw; ++bx) {
          maybe_rst();
          int32_t* blk = &c.coef[((size_t)by * c.bw + bx) * 64];
          decode_block(br, c, blk, pred[ci], Ss, Se, Ah, Al);
          ++unit_count;
        }
    }
    // advance main parse position to the marker the reader stopped at
    pos = br.pos;
  }

  int decode_dc_diff(BitReader& br, const Component& c) {
    int t = decode_huff(br, dc[c.td]);
    if (t > 15) throw std::runtime_error("bad DC magnitude category");
    return extend(br.read_bits(t), t);
  }

  void decode_block(BitReader& br, Component& c, int32_t* blk, int& pred,
                    int Ss, int Se, int Ah, int Al) {
    if (!progressive) {
      // baseline: full block (F.2.2)
      pred = wrap_add(pred, decode_dc_diff(br, c));
      blk[0] = pred;
      int k = 1;
      while (k < 64) {
        int rs = decode_huff(br, ac[c.ta]);
        int r = rs >> 4, s = rs & 15;
        if (rs == 0x00) break;
        if (rs == 0xF0) { k += 16; continue; }
        k += r;
        if (k > 63) break;
        blk[k] = extend(br.read_bits(s), s);
        ++k;
      }
      return;
    }
    if (Ss == 0) {
      if (Ah == 0) {  // DC first (G.2.1)
        pred = wrap_add(pred, decode_dc_diff(br, c));
        blk[0] = wrap_shl(pred, Al);
      } else {        // DC refinement
        if (br.read_bit()) blk[0] |= (1 << Al);
      }
      return;
    }
    // AC scans (single component)
    if (Ah == 0) {  // AC first (G.2.2)
      if (eobrun > 0) { --eobrun; return; }
      int k = Ss;
      while (k <= Se) {
        int rs = decode_huff(br, ac[c.ta]);
        int r = rs >> 4, s = rs & 15;
        if (s == 0) {
          if (r < 15) {
            eobrun = (1 << r) - 1;
            if (r) eobrun += br.read_bits(r);
            break;
          }
          k += 16;  // ZRL
          continue;
        }
        k += r;
        if (k > 63) break;
        blk[k] = wrap_shl(extend(br.read_bits(s), s), Al);
        ++k;
      }
    } else {  // AC refinement (G.2.3 / jpeg6b decode_mcu_AC_refine)
      int p1 = 1 << Al, m1 = -(1 << Al);
      int k = Ss;
      if (eobrun == 0) {
        for (; k <= Se; ) {
          int rs = decode_huff(br, ac[c.ta]);
          int r = rs >> 4, s = rs & 15;
          int val = 0;
          if (s == 0) {
            if (r < 15) {
              eobrun = (1 << r);
              if (r) eobrun += br.read_bits(r);
              break;  // EOB logic handled below
            }
            // ZRL: skip 16 zero-history coefficients
          } else {
            val = br.read_bit() ? p1 : m1;
          }
          while (k <= Se) {
            int32_t& co = blk[k];
            if (co != 0) {
              if (br.read_bit() && (co & p1) == 0)
                co = wrap_add(co, (co >= 0) ? p1 : m1);
            } else {
              if (r == 0) {
                if (val) blk[k] = val;
                ++k;
                break;
              }
              --r;
            }
            ++k;
          }
        }
      }
      if (eobrun > 0) {
        // append correction bits to remaining nonzero coefficients
        for (; k <= Se; ++k) {
          int32_t& co = blk[k];
          if (co != 0) {
            if (br.read_bit() && (co & p1) == 0)
              co = wrap_add(co, (co >= 0) ? p1 : m1);
          }
        }
        --eobrun;
      }
    }
  }

  // Geometry every reconstruction indexes with.  The host reconstruction
  // reads plane 1/2 at (y / (vmax / v), x / (hmax / h)) and plane 0 at
  // (y, x): a second component without a third, a luma plane smaller than
  // the frame, or a factor that does not divide the maximum all read out
  // of bounds, so both entry points reject them here.
  void check_reconstructible() const {
    if (W <= 0 || H <= 0 || comps.empty())
      throw std::runtime_error("no frame decoded");
    if (comps.size() == 2)
      throw std::runtime_error("unsupported component count");
    const size_t used = std::min<size_t>(comps.size(), 3);
    for (size_t i = 0; i < used; ++i) {
      const Component& c = comps[i];
      if (hmax % c.h || vmax % c.v)
        throw std::runtime_error("sampling factor does not divide the MCU");
    }
    if (comps[0].h != hmax || comps[0].v != vmax)
      throw std::runtime_error("first component is subsampled");
  }
};

// One image's entropy-decoded state in the layout the device kernel reads.
struct CompGeom {
  int h = 0, v = 0, tq = 0, bw = 0, bh = 0;
  int64_t block_off = 0;  // first block of this plane in Exported::coef
};

struct Exported {
  int W = 0, H = 0, nc = 0;
  CompGeom comp[3];
  int64_t blocks = 0;
  uint16_t qt[4][64] = {};
  std::vector<int16_t> coef;  // (blocks, 64), zigzag order, planes in order
};

// Validates everything a device reconstruction indexes with and narrows the
// coefficients to int16.  Throws std::runtime_error otherwise.
inline void export_coefficients(const Decoder& dec, Exported& out) {
  dec.check_reconstructible();
  if (dec.precision != 8)
    throw std::runtime_error("unsupported sample precision");
  const int nc = (int)dec.comps.size();
  if (nc != 1 && nc != 3)
    throw std::runtime_error("unsupported component count");
  if ((int64_t)dec.W * dec.H > MAX_PIXELS)
    throw std::runtime_error("unsupported frame size");
  out.W = dec.W;
  out.H = dec.H;
  out.nc = nc;
  int64_t blocks = 0;
  for (int ci = 0; ci < nc; ++ci) {
    const Component& c = dec.comps[ci];
    if (c.h < 1 || c.h > 4 || c.v < 1 || c.v > 4)
      throw std::runtime_error("bad sampling factor");
    if (c.tq < 0 || c.tq > 3)
      throw std::runtime_error("bad quantisation table id");
    CompGeom& g = out.comp[ci];
    g.h = c.h; g.v = c.v; g.tq = c.tq; g.bw = c.bw; g.bh = c.bh;
    g.block_off = blocks;
    blocks += (int64_t)c.bw * c.bh;
  }
  out.blocks = blocks;
  std::memcpy(out.qt, dec.qt, sizeof(out.qt));
  out.coef.resize((size_t)blocks * 64);
  int16_t* dst = out.coef.data();
  for (int ci = 0; ci < nc; ++ci) {
    const std::vector<int32_t>& src = dec.comps[ci].coef;
    for (size_t i = 0; i < src.size(); ++i) {
      const int32_t v = src[i];
      if (v < -32768 || v > 32767)
        throw std::runtime_error("coefficient does not fit int16");
      *dst++ = (int16_t)v;
    }
  }
}

}  // namespace jpegparse
