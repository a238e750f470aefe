// Host-only run of the progressive coders (attwarp_amd/csrc/jpegprogenc_blocks.hpp: the text the jpegprogenc_* kernels run) for
// tests/test_jpegprogenc_host_cpu.py, compiled with -fsanitize=address,undefined.  stdin: n, then n records:
//   scan slot ss se ah al nrows   then nrows x (count, 64 zigzag coefficients): `count` copies of the block in a row.
//        One interval over those blocks (a grey walk, a block per MCU): the statistics pass into a token list and a histogram,
//        the table of the histogram (jo_optimal_table on one lane), the second pass into a buffer of exactly the planner's
//        bound on the heap.  Prints "tokens" (0 slot symbol | 1 value nbits ...), "bytes" (count, then the stuffed bytes).
//        The same interval is then coded BLOCK BY BLOCK as the kernels do (pe_summary, pe_resolve_step, pe_code_block), the
//        blocks in descending order, every block with a state filled with garbage first: the tokens must be the same.
//   dc bpm ny nrows   then the rows as above: the blocks of whole MCUs (ny luma blocks, then Cb, Cr) of an interleaved DC first
//        pass at Al = 1, slot 0 and the chroma slot; tokens of the one walk, which the block-by-block tokens must equal.
//   walk bpm ny hmax vmax mcus_x comp wc n: prints "walk" and per block j < n its component and block index (offset / 64).
// Last line "jpegprogenc_host ok n".
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "jpegprogenc_blocks.hpp"

using namespace attwarp;

struct TokenSink {
  std::vector<long long>* tokens;
  uint32_t* hist;                      // [PE_SLOTS][256]
  void sym(int slot, int s) {
    tokens->insert(tokens->end(), {0, slot, s});
    ++hist[slot * 256 + (s & 255)];
  }
  void bits(uint32_t v, int n) { tokens->insert(tokens->end(), {1, (long long)v, n}); }
};

// the interval block by block, as the kernels code it; false: not the tokens of the one walk
static bool same_block_by_block(const PeWalk& w, const PeScan& sc, int slot, int64_t nblk, const std::vector<long long>& want) {
  std::vector<uint8_t> summary((size_t)nblk);              // exactly nblk bytes on the heap
  std::vector<PeRun> pre((size_t)nblk);
  PeRun r = {0u, 0u};
  for (int64_t j = 0; j < nblk; ++j) {
    int ci;
    summary[(size_t)j] = sc.ss ? (uint8_t)pe_summary(w.block(j, ci), sc) : 0;
    pre[(size_t)j] = r;
    if (sc.ss) pe_resolve_step(summary[(size_t)j], r);
  }
  std::vector<std::vector<long long>> per((size_t)nblk);
  std::vector<uint32_t> hist(PE_SLOTS * 256, 0u);
  auto st = std::make_unique<PeState>();
  for (int64_t j = nblk - 1; j >= 0; --j) {
    std::memset(st.get(), 0xA5, sizeof(PeState));
    TokenSink ts = {&per[(size_t)j], hist.data()};
    pe_code_block(w, sc, slot, 0, nblk, j, summary.data(), pre[(size_t)j], *st, ts);
  }
  std::vector<long long> got;
  for (const auto& v : per) got.insert(got.end(), v.begin(), v.end());
  return got == want;
}

int main() {
  int n = 0;
  if (scanf("%d", &n) != 1 || n < 1 || n > 100000) { fprintf(stderr, "jpegprogenc_host: bad count\n"); return 2; }
  for (int i = 0; i < n; ++i) {
    char mode[16];
    if (scanf("%15s", mode) != 1) { fprintf(stderr, "jpegprogenc_host: record %d\n", i); return 2; }
    if (!strcmp(mode, "walk")) {
      PeWalk w;
      int count;
      static const int16_t origin[1] = {0};
      w.coef = origin;
      if (scanf("%d %d %d %d %d %d %d %d", &w.bpm, &w.ny, &w.hmax, &w.vmax, &w.mcus_x, &w.comp, &w.wc, &count) != 8) return 2;
      printf("walk");
      for (int j = 0; j < count; ++j) {
        int ci = -9;
        const long long at = (w.block(j, ci) - origin) / 64;
        printf(" %d %lld", ci, at);
      }
      printf("\n");
      continue;
    }
    int slot = 0, nrows, bpm = 1, ny = 1;
    PeScan sc = {0, 0, 0, 0, 1};
    const bool dc = !strcmp(mode, "dc");
    if (dc ? scanf("%d %d %d", &bpm, &ny, &nrows) != 3 || bpm < 3 || ny != bpm - 2 || nrows < 1
           : strcmp(mode, "scan") || scanf("%d %d %d %d %d %d", &slot, &sc.ss, &sc.se, &sc.ah, &sc.al, &nrows) != 6 || slot < 0 ||
                 slot >= PE_SLOTS || nrows < 1) {
      fprintf(stderr, "jpegprogenc_host: record %d\n", i);
      return 2;
    }
    if (dc) sc.comp = -1;
    std::vector<int16_t> coef;                              // exactly the blocks on the heap: a read behind them is seen
    for (int r = 0; r < nrows; ++r) {
      int count, v[64];
      if (scanf("%d", &count) != 1 || count < 1 || count > 100000) return 2;
      for (int k = 0; k < 64; ++k)
        if (scanf("%d", &v[k]) != 1 || v[k] < -32768 || v[k] > 32767) return 2;
      for (int c = 0; c < count; ++c)
        for (int k = 0; k < 64; ++k) coef.push_back((int16_t)v[k]);
    }
    const int64_t nblk = (int64_t)coef.size() / 64;
    if (dc && nblk % bpm) return 2;
    PeWalk w = {coef.data(), bpm, ny, ny > 1 ? 2 : 1, ny > 2 ? 2 : 1, (int)(nblk / bpm), sc.comp, (int)nblk};
    std::vector<long long> tokens;
    std::vector<uint32_t> hist(PE_SLOTS * 256, 0u);
    auto st = std::make_unique<PeState>();
    std::memset(st.get(), 0xA5, sizeof(PeState));            // what the kernel's uninitialised state may hold
    TokenSink ts = {&tokens, hist.data()};
    pe_code_interval(w, sc, slot, 0, nblk, *st, ts);
    printf("tokens");
    for (long long t : tokens) printf(" %lld", t);
    printf("\n");
    if (!same_block_by_block(w, sc, slot, nblk, tokens)) { fprintf(stderr, "jpegprogenc_host: record %d: block by block differs\n", i); return 3; }
    if (dc) continue;
    std::vector<JoTable> tables(PE_SLOTS);
    std::memset(tables.data(), 0, tables.size() * sizeof(JoTable));
    auto work = std::make_unique<JoWork>();
    jo_optimal_table<1>(hist.data() + 256 * slot, 0x10, 0, JoOneLane(), *work, tables[slot]);
    const uint32_t cap = (uint32_t)pe_interval_bytes((uint64_t)nblk, pe_block_bits(sc));
    std::vector<uint8_t> out(cap);
    PeByteSink bs = {tables.data(), out.data(), cap, 0, 0, 0};
    pe_code_interval(w, sc, slot, 0, nblk, *st, bs);
    bs.finish();
    if (bs.n > cap) { fprintf(stderr, "jpegprogenc_host: record %d: %u bytes above the bound %u\n", i, bs.n, cap); return 3; }
    printf("bytes %u", bs.n);
    for (uint32_t k = 0; k < bs.n; ++k) printf(" %d", out[k]);
    printf("\n");
  }
  printf("jpegprogenc_host ok %d\n", n);
  return 0;
}
