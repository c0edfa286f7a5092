// The serial decode text of the device PNG reader, run on the host: this program compiles univs_amd/csrc/png_inflate_core.h, the very
// header csrc/png_inflate.hip compiles, with a one-lane copy in place of the wave's.  It is the CPU evidence that the bounds decisions
// hold before any malformed byte reaches a GPU: built with -fsanitize=address,undefined, every stream and the output live in heap blocks
// of exactly their sizes, so a load or store outside a frame's regions is a sanitizer report (tests/test_png_read_cpu.py).
//
//   png_inflate_host EXPECT FILE [EXPECT FILE ...]     each FILE holds one zlib stream that should inflate to EXPECT bytes
//   png_inflate_host -                                   records from stdin: uint64 EXPECT, uint64 LENGTH (little endian), LENGTH bytes
//
// One line per stream: "<status> <bytes produced> <FNV-1a 64 of the produced bytes, hex>"; the status is PngStatus.
//   c++ -O1 -g -std=c++17 [-fsanitize=address,undefined] tools/png_inflate_host.cpp -o png_inflate_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../univs_amd/csrc/png_inflate_core.h"

struct OneLane {
  static constexpr int N = 1;
  static int lane() { return 0; }
  static void sync() {}
};

static void run(const std::vector<unsigned char>& stream, unsigned long long expect) {
  // exact heap blocks: the sanitizer sees the first byte outside either
  unsigned char* in = static_cast<unsigned char*>(std::malloc(stream.size() ? stream.size() : 1));
  unsigned char* out = static_cast<unsigned char*>(std::malloc(expect ? expect : 1));
  unsigned char* ring = static_cast<unsigned char*>(std::malloc(univs::PNG_WINDOW));
  univs::PngTables* tables = static_cast<univs::PngTables*>(std::malloc(sizeof(univs::PngTables)));
  unsigned long long red[4];
  if (!in || !out || !ring || !tables) {
    std::fprintf(stderr, "png_inflate_host: out of memory\n");
    std::exit(2);
  }
  if (!stream.empty()) std::memcpy(in, stream.data(), stream.size());
  std::memset(ring, 0, univs::PNG_WINDOW);
  long long produced = 0;
  const int status = univs::png_inflate<OneLane>(in, 0, (long long)stream.size(), out, (long long)expect, ring, tables, red, &produced);
  unsigned long long h = 1469598103934665603ull;
  for (long long i = 0; i < produced; ++i) h = (h ^ out[i]) * 1099511628211ull;
  std::printf("%d %lld %016llx\n", status, produced, h);
  std::free(in), std::free(out), std::free(ring), std::free(tables);
}

static bool read_exact(std::FILE* f, void* dst, size_t n) { return std::fread(dst, 1, n, f) == n; }

static unsigned long long le64(const unsigned char* p) {
  unsigned long long v = 0;
  for (int i = 7; i >= 0; --i) v = (v << 8) | p[i];
  return v;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "-") == 0) {
    unsigned char head[16];
    while (read_exact(stdin, head, 16)) {
      const unsigned long long expect = le64(head), len = le64(head + 8);
      if (expect >= (1ull << 31) || len >= (1ull << 31)) {
        std::fprintf(stderr, "png_inflate_host: record of %llu -> %llu bytes\n", len, expect);
        return 2;
      }
      std::vector<unsigned char> s(len);
      if (len && !read_exact(stdin, s.data(), len)) {
        std::fprintf(stderr, "png_inflate_host: short record\n");
        return 2;
      }
      run(s, expect);
    }
    return 0;
  }
  if (argc < 3 || (argc - 1) % 2) {
    std::fprintf(stderr, "usage: png_inflate_host EXPECT FILE [EXPECT FILE ...]  |  png_inflate_host - < records\n");
    return 2;
  }
  for (int i = 1; i + 1 < argc; i += 2) {
    std::FILE* f = std::fopen(argv[i + 1], "rb");
    if (!f) {
      std::fprintf(stderr, "png_inflate_host: cannot open %s\n", argv[i + 1]);
      return 2;
    }
    std::vector<unsigned char> s;
    unsigned char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) s.insert(s.end(), buf, buf + n);
    std::fclose(f);
    run(s, std::strtoull(argv[i], nullptr, 10));
  }
  return 0;
}
