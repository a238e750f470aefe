// Host-only check of the PNG encoder's shared host / device pieces (attwarp_amd/csrc/png_blocks.hpp) for
// tests/test_png_host_cpu.py: the same text the kernels run, compiled for the CPU with -fsanitize=address,undefined.
//   png_length_symbol     every match length 3 .. 258 against RFC 1951's table of bases and extra bits, written out here;
//   png_filter            the specification's five formulas over every (left, up, upper left) and a few current bytes;
//   crc_mulmod / crc_xpow8 / crc_table_entry / crc_bytes
//                         against a plain bitwise CRC-32: one CRC per lane over 256 equal slices, shifted to the end and XORed,
//                         as the encode kernel cuts a segment, and through the assemble kernel's combine of head, segments
//                         and trailer;
//   png_rows_per_segment  at the row sizes where it changes.
// Every buffer is exactly as long as its data, so the sanitizer sees any byte read outside it.  Prints one line and returns 0.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "png_blocks.hpp"

using namespace attwarp;

static int bad(const char* what, long a, long b, long c) {
  fprintf(stderr, "png_host: %s at %ld %ld %ld\n", what, a, b, c);
  return 3;
}

// RFC 1951 3.2.5: length codes 257 .. 285
static const int RFC_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const int RFC_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};

static uint32_t plain_crc(const uint8_t* p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
  }
  return c ^ 0xffffffffu;
}

// the specification's filters, section 9.2 and 9.4
static int spec_paeth(int a, int b, int c) {
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  if (pa <= pb && pa <= pc) return a;
  if (pb <= pc) return b;
  return c;
}
static uint32_t spec_filter(int ft, int x, int a, int b, int c) {
  int pred = 0;
  switch (ft) {
    case 0: pred = 0; break;
    case 1: pred = a; break;
    case 2: pred = b; break;
    case 3: pred = (a + b) / 2; break;
    default: pred = spec_paeth(a, b, c); break;
  }
  return (uint32_t)((x - pred) % 256 + 256) % 256;
}

static uint32_t rnd(uint32_t& s) { return (s = s * 1664525u + 1013904223u) >> 24; }

// CRC-32 of d[0 .. n) as a workgroup of the encode kernel computes it: 256 lanes of ceil(n / 256) bytes
static uint32_t sliced_crc(const uint8_t* d, uint32_t n, const uint32_t* table, const uint32_t* pow8) {
  const uint32_t L = (n + PNG_NT - 1) / PNG_NT;
  uint32_t x = 0;
  for (uint32_t t = 0; t < (uint32_t)PNG_NT; ++t) {
    const uint32_t b0 = n < t * L ? n : t * L, b1 = n < b0 + L ? n : b0 + L;
    uint32_t c = 0xffffffffu;
    for (uint32_t i = b0; i < b1; ++i) c = table[(c ^ d[i]) & 255u] ^ (c >> 8);
    c = ~c;
    if (b0 == b1) c = 0;
    x ^= crc_mulmod(c, crc_xpow8(n - b1, pow8));
  }
  return x;
}

int main() {
  long checks = 0;
  // ---- length symbols ---------------------------------------------------------------------------------------------------
  for (uint32_t L = 3; L <= 258; ++L) {
    int k = 28;
    while (RFC_BASE[k] > (int)L) --k;
    uint32_t sym = 0, eb = 99, ev = 99;
    png_length_symbol(L, sym, eb, ev);
    if (sym != 257u + (uint32_t)k || eb != (uint32_t)RFC_EXTRA[k] || ev != L - (uint32_t)RFC_BASE[k] || ev >= (1u << eb)) return bad("length symbol", L, sym, ev);
    ++checks;
  }
  // ---- filters ----------------------------------------------------------------------------------------------------------
  const int curs[3] = {0, 128, 255};
  for (int a = 0; a < 256; ++a)
    for (int b = 0; b < 256; ++b)
      for (int c = 0; c < 256; ++c)
        for (int ft = 0; ft < 5; ++ft)
          for (int x : curs) {
            if (png_filter(ft, x, a, b, c) != spec_filter(ft, x, a, b, c)) return bad("filter", ft, a * 65536L + b * 256 + c, x);
            ++checks;
          }
  for (int x = 0; x < 256; ++x)
    for (int a = 0; a < 256; ++a)
      for (int ft = 0; ft < 5; ++ft) {
        if (png_filter(ft, x, a, 255 - a, (a * 7 + x) & 255) != spec_filter(ft, x, a, 255 - a, (a * 7 + x) & 255)) return bad("filter (every current byte)", ft, a, x);
        ++checks;
      }
  // ---- CRC-32 -----------------------------------------------------------------------------------------------------------
  uint32_t table[256], pow8[32], p = 0x40000000u;          // x^1; the planner's table of x^(8 * 2^k)
  for (uint32_t n = 0; n < 256; ++n) table[n] = crc_table_entry(n);
  for (int k = 0; k < 3; ++k) p = crc_mulmod(p, p);
  for (int k = 0; k < 32; ++k) { pow8[k] = p; p = crc_mulmod(p, p); }
  if (crc_xpow8(0u, pow8) != 0x80000000u || crc_xpow8(1u, pow8) != pow8[0]) return bad("xpow8", 0, 0, 0);
  if (crc_mulmod(0x80000000u, 0x12345678u) != 0x12345678u || crc_mulmod(0x12345678u, 0x80000000u) != 0x12345678u) return bad("mulmod by one", 0, 0, 0);
  const uint32_t lens[7] = {0, 1, 255, 256, 257, 159, 24581};
  uint32_t seed = 12345u;
  std::vector<std::vector<uint8_t>> segs;
  for (uint32_t n : lens) {
    std::vector<uint8_t> d(n);
    for (auto& v : d) v = (uint8_t)rnd(seed);
    const uint32_t want = plain_crc(d.data(), n);
    if (crc_bytes(d.data(), (int)n) != want) return bad("crc_bytes", n, 0, 0);
    if (sliced_crc(d.data(), n, table, pow8) != want) return bad("sliced crc", n, 0, 0);
    if (n >= 2 && crc_bytes(d.data() + n / 3, (int)(n - n / 3), crc_bytes(d.data(), (int)(n / 3))) != want) return bad("crc_bytes continued", n, 0, 0);
    segs.push_back(d);
    checks += 3;
  }
  // the assemble kernel's combine: IDAT + zlib header, the segments (each shifted by what stands behind it), nine trailer bytes
  for (int rot = 0; rot < 7; ++rot) {
    const uint8_t head[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
    const uint8_t tail[9] = {0x01, 0x00, 0x00, 0xff, 0xff, (uint8_t)(17 * rot), 0xbe, 0xef, 0x42};
    std::vector<uint8_t> all(head, head + 6);
    uint32_t total = 0;
    for (int s = 0; s < 7; ++s) total += (uint32_t)segs[(s + rot) % 7].size();
    uint32_t x = 0, pre = 0;
    for (int s = 0; s < 7; ++s) {
      const std::vector<uint8_t>& d = segs[(s + rot) % 7];
      const uint32_t len = (uint32_t)d.size();
      x ^= crc_mulmod(sliced_crc(d.data(), len, table, pow8), crc_xpow8(total - pre - len + 9u, pow8));
      pre += len;
      all.insert(all.end(), d.begin(), d.end());
    }
    all.insert(all.end(), tail, tail + 9);
    const uint32_t got = crc_mulmod(crc_bytes(head, 6), crc_xpow8(total + 9u, pow8)) ^ x ^ crc_bytes(tail, 9);
    if (got != plain_crc(all.data(), all.size())) return bad("crc combine", rot, total, 0);
    ++checks;
  }
  // ---- rows per segment ---------------------------------------------------------------------------------------------------
  const int rows[8][2] = {{2, 1024}, {24, 1024}, {25, 983}, {12288, 2}, {12289, 1}, {24576, 1}, {23, 1024}, {8192, 3}};
  for (auto& r : rows) {
    if (png_rows_per_segment(r[0]) != r[1]) return bad("rows per segment", r[0], png_rows_per_segment(r[0]), r[1]);
    ++checks;
  }
  printf("png_host ok %ld\n", checks);
  return 0;
}
