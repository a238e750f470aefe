// Host-only driver of the PNG decoder's wave route (attwarp_amd/csrc/pngdec_wave_blocks.hpp) for
// tests/test_pngwave_host_cpu.py: the same text the kernel runs, the 64 lanes one after the other in place of the wave,
// compiled for the CPU with -fsanitize=address,undefined.  Usage: pngwave_host CORPUS SEGMENT_BYTES MAX_ROUNDS.  Reads a corpus
//   u32 nfiles, then per file: u32 filt_bytes, u32 row_bytes, u32 nchunks, nchunks x (u32 len, u32 crc), the IDAT payloads
// and prints per file: windows, rounds, accepted, resolution rounds, and the Adler-32 of the filtered bytes (0 unless accepted).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pngdec_wave_blocks.hpp"

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
  if (argc != 4) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const uint32_t seg = (uint32_t)atoi(argv[2]), mr = (uint32_t)atoi(argv[3]);
  if (!(seg == 16 || seg == 32 || seg == 64 || seg == 128 || seg == 256) || mr < 1 || mr > 64) return 2;
  PwShared* S = new PwShared;
  const uint32_t nfiles = rd32(f);
  for (uint32_t i = 0; i < nfiles; ++i) {
    const uint32_t filt_bytes = rd32(f);
    rd32(f);
    const uint32_t nchunks = rd32(f);
    size_t total = 0;
    for (uint32_t c = 0; c < nchunks; ++c) { total += rd32(f); rd32(f); }
    // exactly as long as the stream and the image: the sanitizer sees any byte read or written outside them
    std::vector<uint8_t> s(total), filt(filt_bytes);
    if (total && fread(s.data(), 1, total, f) != total) return 2;
    PwRecord rec = {0, 0, 0, 0};
    uint32_t adler_pos = 0, adler = 0;
    if (pd_zlib_header(s.data(), (uint32_t)total) == 0) {     // (the kernel runs only for images whose header the scan accepted)
      pw_image(*S, s.data(), (uint32_t)total, filt.data(), filt_bytes, seg, mr, &rec, &adler_pos);
      if (rec.accepted) {
        adler = adler_of(filt.data(), filt_bytes);
        if (adler_pos + 4 > total) { fprintf(stderr, "file %u: accepted with the Adler-32 outside the stream\n", i); return 3; }
      }
    }
    printf("%u %u %u %u %u\n", rec.windows, rec.rounds, rec.accepted, rec.resolution_rounds, adler);
  }
  delete S;
  fclose(f);
  return 0;
}
