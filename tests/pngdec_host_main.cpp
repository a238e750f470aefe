// Host-only driver of the PNG decoder's shared core (attwarp_amd/csrc/pngdec_blocks.hpp) for tests/test_pngdec_host_cpu.py:
// the same text the kernels run, compiled for the CPU with -fsanitize=address,undefined.  Reads a corpus file
//   u32 nfiles, then per file: u32 filt_bytes, u32 row_bytes, u32 nchunks, nchunks x (u32 len, u32 crc), the IDAT payloads
// and prints per file: status, Adler-32 of the filtered bytes produced, route (0 unit, 1 serial, 2 none), units on the
// chain, kept positions.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pngdec_blocks.hpp"

using namespace attwarp;

static uint32_t rd32(FILE* f) {
  uint8_t b[4];
  if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "short corpus\n"); exit(2); }
  return b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}

static uint32_t adler_of(const uint8_t* d, uint32_t n) {
  unsigned long long a = 0, w = 0;
  for (uint32_t i = 0; i < n; ++i) { a += d[i]; w = (w + (unsigned long long)d[i] * ((n - i) % PNG_ADLER)) % PNG_ADLER; }
  return pd_adler_finish(a % PNG_ADLER, w, n);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  // the inverse tables against the encoder's png_length_symbol
  for (uint32_t L = 3; L <= 258; ++L) {
    uint32_t sym, eb, ev, base, eb2;
    png_length_symbol(L, sym, eb, ev);
    pd_length_base(sym - 257, base, eb2);
    if (base + ev != L || eb != eb2) { fprintf(stderr, "length table mismatch at %u\n", L); return 3; }
  }
  uint32_t pow8[32], p = 0x40000000u;
  for (int k = 0; k < 3; ++k) p = crc_mulmod(p, p);
  for (int k = 0; k < 32; ++k) { pow8[k] = p; p = crc_mulmod(p, p); }
  const uint8_t idat[4] = {'I', 'D', 'A', 'T'};
  const uint32_t idat_crc = crc_bytes(idat, 4);
  const uint32_t nfiles = rd32(f);
  for (uint32_t i = 0; i < nfiles; ++i) {
    const uint32_t filt_bytes = rd32(f), row_bytes = rd32(f), nchunks = rd32(f);
    std::vector<uint32_t> len(nchunks), crc(nchunks);
    size_t total = 0;
    for (uint32_t c = 0; c < nchunks; ++c) { len[c] = rd32(f); crc[c] = rd32(f); total += len[c]; }
    // exactly as long as the stream and the image: the sanitizer sees any byte read or written outside them
    std::vector<uint8_t> s(total), filt(filt_bytes);
    if (total && fread(s.data(), 1, total, f) != total) return 2;
    const uint32_t n = (uint32_t)total;
    uint32_t st_crc = 0;
    size_t off = 0;
    for (uint32_t c = 0; c < nchunks; ++c) {
      const uint32_t got = crc_mulmod(idat_crc, crc_xpow8(len[c], pow8)) ^ crc_bytes(s.data() + off, (int)len[c]);
      if (got != crc[c]) st_crc = ATTWARP_PNGDEC_E_CRC;
      off += len[c];
    }
    uint32_t st = pd_zlib_header(s.data(), n), route = 2, chain_len = 0, produced = 0, adler_pos = 0;
    std::vector<uint32_t> kept;
    if (st == 0) {
      kept.push_back(2u);
      for (uint32_t q = 2; q + 5 <= n && kept.size() < (size_t)PD_MAX_UNITS; ++q)
        if (s[q] == 0 && s[q + 1] == 0 && s[q + 2] == 0xff && s[q + 3] == 0xff) kept.push_back(q + 4);
      const uint32_t nunits = (uint32_t)kept.size();
      PdTables* tb = new PdTables;
      std::vector<PdUnit> units(nunits);
      route = 1;
      if (nunits > 1) {
        for (uint32_t u = 0; u < nunits; ++u) {
          const PdResult r = pd_inflate(s.data(), n, kept[u], nullptr, filt_bytes, kept.data(), nunits, *tb);
          units[u] = PdUnit{kept[u], r.end, r.out_len, 0, r.status, r.final, r.dependent, 0};
        }
        if (pd_chain(units.data(), nunits, filt_bytes, n, adler_pos, chain_len)) route = 0;
      }
      if (route == 0) {
        for (uint32_t u = 0; u < nunits; ++u) {
          if (!units[u].on_chain) continue;
          const PdResult r = pd_inflate(s.data(), n, units[u].start, filt.data() + units[u].out_off, units[u].out_len, kept.data(), nunits, *tb);
          if (r.status || r.out_len != units[u].out_len || r.end != units[u].end) st = r.status ? r.status : (uint32_t)ATTWARP_PNGDEC_E_UNDERFLOW;
        }
        produced = filt_bytes;
      } else {
        chain_len = 0;
        const PdResult r = pd_inflate(s.data(), n, 2, filt.data(), filt_bytes, nullptr, 0, *tb);
        st = pd_serial_status(r, filt_bytes, n);
        produced = r.out_len;
        adler_pos = r.end;
      }
      delete tb;
    }
    const uint32_t adler = adler_of(filt.data(), produced);
    if (st == 0 && pd_be32(s.data() + adler_pos) != adler) st = ATTWARP_PNGDEC_E_ADLER;
    if (st == 0)
      for (uint32_t r = 0; r < filt_bytes / row_bytes; ++r)
        if (filt[(size_t)r * row_bytes] > 4) st = ATTWARP_PNGDEC_E_FILTER;
    printf("%u %u %u %u %zu\n", st_crc ? st_crc : st, adler, route, chain_len, kept.size());
  }
  fclose(f);
  return 0;
}
