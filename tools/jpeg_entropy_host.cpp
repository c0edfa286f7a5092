// The entropy decoder of the device JPEG reader, run on the host: this program compiles univs_amd/csrc/jpeg_entropy_core.h, the very header
// csrc/jpeg_decode.hip compiles, and runs it twice per file: serially (one span per restart interval), and by the kernel's subsequence
// schedule, lane by lane: phase 1 (every lane from the default state), phase 2 (lane i + 1 again from lane i's exit until no start
// changes, a counted loop), phase 3 (scans, then the write pass), in chunks of JPEG_WG lanes.  It is the CPU evidence for the parallel
// algorithm and for the bounds decisions: built with -fsanitize=address,undefined, every interval's bytes and the block buffer live in
// heap blocks of exactly their sizes, so a load or store outside them is a sanitizer report (tests/test_jpeg_entropy_cpu.py).
//
//   jpeg_entropy_host < records
// A record (little endian): int32 per, hv, ri (MCUs per restart interval), mcus, subseq_bits, ntab; ntab x 272 table bytes (16 counts, 256
// values; [2 c] DC and [2 c + 1] AC of component c); uint64 LENGTH; LENGTH bytes: the file from the end of the SOS header on.
// One line per record:
//   <serial status> <schedule status> <blocks> <FNV-1a 64 of the serial blocks> <... of the schedule's> <most rounds of a chunk>
//   <most lanes of a chunk> <1: every lane's exit state is the serial decode's at that bit position>
//   c++ -O1 -g -std=c++17 [-fsanitize=address,undefined] tools/jpeg_entropy_host.cpp -o jpeg_entropy_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../univs_amd/csrc/jpeg_entropy_core.h"

using namespace univs;

static uint8_t kZigzag[64];

struct Interval {
  uint8_t* bytes;   // an exact heap block
  int nbytes;
};

// The pre-pass: the kept bytes of each interval, and the status bits of the markers
static int prepass(const std::vector<uint8_t>& raw, std::vector<Interval>* out) {
  std::vector<uint8_t> cur;
  int status = 0, nrst = 0;
  bool ended = false;
  auto close = [&]() {
    Interval iv{static_cast<uint8_t*>(std::malloc(cur.empty() ? 1 : cur.size())), (int)cur.size()};
    if (!cur.empty()) std::memcpy(iv.bytes, cur.data(), cur.size());
    out->push_back(iv);
    cur.clear();
  };
  for (size_t i = 0; i < raw.size(); ++i) {
    const unsigned prev = i ? raw[i - 1] : 0u, next = i + 1 < raw.size() ? raw[i + 1] : 0x100u;
    const int role = jpeg_byte_role(prev, raw[i], next);
    if (role == JPEG_KEEP) cur.push_back(raw[i]);
    if (role == JPEG_RST) {
      if ((int)(next - 0xD0) != (nrst & 7)) status |= JPEG_ERR_RESTART;
      ++nrst;
      close();
    }
    if (role == JPEG_END) {
      if (next != 0xD9) status |= JPEG_ERR_EOI;
      ended = true;
      break;
    }
  }
  if (!ended) status |= JPEG_ERR_EOI;
  close();
  return status;
}

struct Problem {
  int per, hv, ri, mcus, subseq_bits, ntab;
  JpegTable tab[6];
  bool tables_ok;
};

static unsigned long long fnv(const int16_t* b, long long n) {
  const unsigned char* p = reinterpret_cast<const unsigned char*>(b);
  unsigned long long h = 1469598103934665603ull;
  for (long long i = 0; i < n * 2; ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

static bool same_pbz(const JpegState& a, const JpegState& b) { return a.p == b.p && a.b == b.b && a.z == b.z; }

static JpegState fresh(int p, int b, int z) { return JpegState{p, b, z, 0, {0, 0, 0}, 0}; }

// One interval by the schedule; returns status bits
static int schedule(const Problem& pr, const JpegScan& sc, int16_t* blocks, long long nblocks, long long base, int limit, int* most_rounds,
                    int* most_lanes, bool* states_ok) {
  const int nbits = sc.nbytes * 8, sb = pr.subseq_bits;
  const int nsub = (nbits + sb - 1) / sb;
  int status = 0;
  JpegState carry = fresh(0, 0, 0);                                 // p, b, z of the chunk's first lane; n, dc: the interval's totals so far
  JpegState truth = fresh(0, 0, 0);                                 // the serial decode, span by span
  std::vector<JpegState> start(JPEG_WG), exitst(JPEG_WG), next(JPEG_WG);
  for (int c0 = 0; c0 < nsub; c0 += JPEG_WG) {
    const int na = nsub - c0 < JPEG_WG ? nsub - c0 : JPEG_WG;
    if (na > *most_lanes) *most_lanes = na;
    auto span_end = [&](int i) { return (c0 + i + 1) * sb < nbits ? (c0 + i + 1) * sb : nbits; };
    // phase 1
    for (int i = 0; i < na; ++i) {
      start[i] = i == 0 ? fresh(carry.p, carry.b, carry.z) : fresh((c0 + i) * sb, 0, 0);
      exitst[i] = start[i];
      jpeg_decode_span<false>(sc, exitst[i], span_end(i), nullptr, 0, 0, 0, nullptr);
    }
    // phase 2: at most na - 1 rounds
    int rounds = 0;
    for (int r = 1; r < na; ++r) {
      bool changed = false;
      next = exitst;
      for (int i = 1; i < na; ++i) {
        if (same_pbz(exitst[i - 1], start[i])) continue;
        start[i] = fresh(exitst[i - 1].p, exitst[i - 1].b, exitst[i - 1].z);
        next[i] = start[i];
        jpeg_decode_span<false>(sc, next[i], span_end(i), nullptr, 0, 0, 0, nullptr);
        changed = true;
      }
      exitst = next;
      ++rounds;
      if (!changed) break;
    }
    if (rounds > *most_rounds) *most_rounds = rounds;
    // the fixpoint against the serial decode
    for (int i = 0; i < na; ++i) {
      JpegState t = fresh(truth.p, truth.b, truth.z);
      jpeg_decode_span<false>(sc, t, span_end(i), nullptr, 0, 0, 0, nullptr);
      if (!same_pbz(t, exitst[i]) || t.n != exitst[i].n || t.err != exitst[i].err || std::memcmp(t.dc, exitst[i].dc, sizeof t.dc)) *states_ok = false;
      truth = t;
    }
    // phase 3: exclusive scans, then the write pass
    long long n0 = carry.n;
    int dc0[3] = {carry.dc[0], carry.dc[1], carry.dc[2]};
    for (int i = 0; i < na; ++i) {
      JpegState w = i == 0 ? fresh(carry.p, carry.b, carry.z) : fresh(exitst[i - 1].p, exitst[i - 1].b, exitst[i - 1].z);
      const long long owed = (long long)limit - n0;
      if (owed > 0) {
        jpeg_decode_span<true>(sc, w, span_end(i), blocks, nblocks, base + n0, (int)owed, dc0);
        status |= w.err;
      }
      n0 += exitst[i].n;
      for (int c = 0; c < 3; ++c) dc0[c] = (int)((unsigned)dc0[c] + (unsigned)exitst[i].dc[c]);
    }
    carry = exitst[na - 1];
    carry.n = (int)n0;
    for (int c = 0; c < 3; ++c) carry.dc[c] = dc0[c];
  }
  if (carry.n < limit) status |= JPEG_ERR_EXHAUSTED;
  return status;
}

static void run(const Problem& pr, const std::vector<uint8_t>& raw) {
  std::vector<Interval> ivs;
  int st_serial = prepass(raw, &ivs);
  const int ri = pr.ri > 0 ? pr.ri : pr.mcus;
  const int expect = (pr.mcus + ri - 1) / ri;
  if ((int)ivs.size() != expect) st_serial |= JPEG_ERR_RESTART;
  if (!pr.tables_ok) st_serial |= JPEG_ERR_TABLE;
  int st_sched = st_serial;
  const long long nblocks = (long long)pr.mcus * pr.per;
  int16_t* a = static_cast<int16_t*>(std::calloc(nblocks * 64, 2));  // exact heap blocks: the sanitizer sees the first element outside
  int16_t* b = static_cast<int16_t*>(std::calloc(nblocks * 64, 2));
  if (!a || !b) {
    std::fprintf(stderr, "jpeg_entropy_host: out of memory\n");
    std::exit(2);
  }
  int most_rounds = 0, most_lanes = 0;
  bool states_ok = true;
  if (st_serial == 0) {
    for (int k = 0; k < expect; ++k) {
      const JpegScan sc{ivs[k].bytes, ivs[k].nbytes, pr.per, pr.hv, pr.tab, kZigzag};
      const long long base = (long long)k * ri * pr.per;
      const int left = pr.mcus - k * ri;
      const int limit = (left < ri ? left : ri) * pr.per;
      if (ivs[k].nbytes >= JPEG_MAX_INTERVAL) {
        st_serial |= JPEG_ERR_DESC, st_sched |= JPEG_ERR_DESC;
        continue;
      }
      // serially: one span, the write mode from the interval's first bit
      JpegState s = fresh(0, 0, 0);
      const int zero[3] = {0, 0, 0};
      jpeg_decode_span<true>(sc, s, sc.nbytes * 8, a, nblocks, base, limit, zero);
      st_serial |= s.err;
      if (s.n < limit) st_serial |= JPEG_ERR_EXHAUSTED;
      st_sched |= schedule(pr, sc, b, nblocks, base, limit, &most_rounds, &most_lanes, &states_ok);
    }
  }
  std::printf("%d %d %lld %016llx %016llx %d %d %d\n", st_serial, st_sched, nblocks, fnv(a, nblocks * 64), fnv(b, nblocks * 64), most_rounds,
              most_lanes, states_ok ? 1 : 0);
  for (auto& iv : ivs) std::free(iv.bytes);
  std::free(a), std::free(b);
}

static bool read_exact(void* dst, size_t n) { return std::fread(dst, 1, n, stdin) == n; }

int main() {
  for (int z = 0; z < 64; ++z) kZigzag[z] = (uint8_t)jpeg_zigzag(z);
  int32_t head[6];
  while (read_exact(head, sizeof head)) {
    Problem pr{head[0], head[1], head[2], head[3], head[4], head[5], {}, true};
    const bool sane = pr.per >= 1 && pr.per <= JPEG_MAX_PER_MCU && pr.hv >= 1 && pr.hv <= 4 && pr.ntab == 2 * (pr.per - pr.hv + 1) && pr.ri >= 0 &&
                      pr.mcus >= 1 && pr.mcus <= (1 << 22) && pr.subseq_bits >= 32 && pr.subseq_bits % 32 == 0 && pr.subseq_bits <= (1 << 20);
    if (!sane) {
      std::fprintf(stderr, "jpeg_entropy_host: bad record header\n");
      return 2;
    }
    for (int t = 0; t < pr.ntab; ++t) {
      uint8_t src[JPEG_TABLE_BYTES];
      if (!read_exact(src, sizeof src)) return 2;
      pr.tables_ok = jpeg_build_table(src, &pr.tab[t]) && pr.tables_ok;
    }
    unsigned long long len;
    if (!read_exact(&len, 8) || len >= (1ull << 31)) return 2;
    std::vector<uint8_t> raw(len);
    if (len && !read_exact(raw.data(), len)) {
      std::fprintf(stderr, "jpeg_entropy_host: short record\n");
      return 2;
    }
    run(pr, raw);
  }
  return 0;
}
