// Host-only run of the optimised-table builder (attwarp_amd/csrc/jpegopt_blocks.hpp: jo_optimal_table, the text the table
// kernel runs, here on one lane) for tests/test_jpegopt_host_cpu.py, compiled with -fsanitize=address,undefined.
// stdin: n, then n x 256 counts.  Per histogram one line "table i depth nsym", one "dht" with the segment's bytes and one
// "codes" with the 256 code words; every record lies between guard bytes that must survive.  Last line "jpegopt_host ok n".
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "jpegopt_blocks.hpp"

using namespace attwarp;

struct Guarded {
  uint8_t before[64];
  JoTable table;
  uint8_t after[64];
};

int main() {
  int n = 0;
  if (scanf("%d", &n) != 1 || n < 1 || n > 4096) { fprintf(stderr, "jpegopt_host: bad count\n"); return 2; }
  for (int i = 0; i < n; ++i) {
    std::vector<uint32_t> hist(256);                        // exactly 256 counts on the heap: a read behind them is seen
    for (auto& v : hist) {
      unsigned long long x;
      if (scanf("%llu", &x) != 1 || x > 0xffffffffull) { fprintf(stderr, "jpegopt_host: bad count in histogram %d\n", i); return 2; }
      v = (uint32_t)x;
    }
    auto work = std::make_unique<JoWork>();
    auto out = std::make_unique<Guarded>();
    std::memset(out.get(), 0xA5, sizeof(Guarded));
    jo_optimal_table<1>(hist.data(), (i & 1) << 4 | (i >> 1 & 1), 0, JoOneLane(), *work, out->table);
    for (int k = 0; k < 64; ++k)
      if (out->before[k] != 0xA5 || out->after[k] != 0xA5) { fprintf(stderr, "jpegopt_host: guard byte %d of histogram %d\n", k, i); return 3; }
    const JoTable& t = out->table;
    if (t.dht_len < 21 || t.dht_len > JO_DHT_BYTES || t.nsym != t.dht_len - 21) { fprintf(stderr, "jpegopt_host: lengths of table %d\n", i); return 3; }
    printf("table %d %d %d\ndht", i, t.depth, t.nsym);
    for (int k = 0; k < t.dht_len; ++k) printf(" %d", t.dht[k]);
    printf("\ncodes");
    for (int s = 0; s < 256; ++s) printf(" %u", t.code[s]);
    printf("\n");
  }
  printf("jpegopt_host ok %d\n", n);
  return 0;
}
