// Stand-alone harness for the JPEG parser + coefficient export
// (mmlspark_amd/io_http/jpeg_parse.h): no torch, no Python.
//
// Reads every stream file named on the command line, runs parse + export on
// it, and exits 0 if each stream either decoded or threw std::runtime_error.
// Built with the sanitizers it proves that malformed streams are rejected
// instead of corrupting memory:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined \
//       -fno-sanitize-recover=all -I mmlspark_amd/io_http \
//       tools/jpeg_parse_fuzz.cpp -o jpeg_parse_fuzz
//   ./jpeg_parse_fuzz corpus/*.jpg
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <vector>

#include "jpeg_parse.h"

int main(int argc, char** argv) {
  int decoded = 0, rejected = 0;
  for (int i = 1; i < argc; ++i) {
    std::ifstream f(argv[i], std::ios::binary);
    if (!f) {
      std::fprintf(stderr, "cannot read %s\n", argv[i]);
      return 2;
    }
    std::vector<uint8_t> buf((std::istreambuf_iterator<char>(f)),
                             std::istreambuf_iterator<char>());
    // hand the parser an exactly-sized heap copy so the sanitizer sees any
    // read one past the end
    std::vector<uint8_t> exact(buf.begin(), buf.end());
    exact.shrink_to_fit();
    try {
      jpegparse::Decoder dec(exact.data(), exact.size());
      dec.parse();
      jpegparse::Exported ex;
      jpegparse::export_coefficients(dec, ex);
      // what a consumer indexes with must be inside what was exported
      for (int c = 0; c < ex.nc; ++c) {
        const jpegparse::CompGeom& g = ex.comp[c];
        if (g.tq > 3 || g.block_off + (int64_t)g.bw * g.bh > ex.blocks ||
            (int64_t)ex.coef.size() != ex.blocks * 64) {
          std::fprintf(stderr, "%s: inconsistent export\n", argv[i]);
          return 1;
        }
      }
      ++decoded;
    } catch (const std::runtime_error&) {
      ++rejected;
    }
  }
  std::printf("%d streams: %d decoded, %d rejected\n", argc - 1, decoded,
              rejected);
  return 0;
}
