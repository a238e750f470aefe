// Host-only driver of the PNG decoder's format blocks (attwarp_amd/csrc/pngfmt_blocks.hpp) for tests/test_pngfmt_host_cpu.py:
// the same text pngdec_unfilter_formats_kernel runs, compiled for the CPU with -fsanitize=address,undefined.  Reads a corpus
//   u32 nfiles, then per file: u32 W, H, colour type, depth, interlace, palette entries, 768 palette bytes (zero padded),
//   u32 nfilt, the nfilt inflated (still filtered) bytes
// and walks every pass as the kernel does -- unit by unit with pd_recon, the pixels of a unit through pf_pixel / pf_output to
// ((y0 + r dy) W + x0 + x dx) oc -- into buffers exactly as long as the image.  Prints per file: the filtered size, the seven
// pass offsets, and the CRC-32 of the pixels in RGB, L, keep and RGB with order bgr; "filter" in place of the CRCs when a
// filter byte is above 4.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pngfmt_blocks.hpp"

using namespace attwarp;

static uint32_t rd32(FILE* f) {
  uint8_t b[4];
  if (fread(b, 1, 4, f) != 4) { fprintf(stderr, "short corpus\n"); exit(2); }
  return b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const uint32_t nfiles = rd32(f);
  for (uint32_t i = 0; i < nfiles; ++i) {
    const int W = (int)rd32(f), H = (int)rd32(f), ctype = (int)rd32(f), depth = (int)rd32(f), lace = (int)rd32(f);
    (void)rd32(f);
    uint8_t pal[768];
    if (fread(pal, 1, 768, f) != 768) return 2;
    const uint32_t nfilt = rd32(f);
    std::vector<uint8_t> filt(nfilt);
    if (nfilt && fread(filt.data(), 1, nfilt, f) != nfilt) return 2;
    if (!pf_valid(depth, ctype) || lace < 0 || lace > 1) { fprintf(stderr, "file %u: not a format\n", i); return 3; }
    const int ch = pf_channels(ctype), unit = pf_unit(ch, depth), ppu = pf_unit_pixels(depth);
    const int64_t total = pf_pass_offset(lace, PF_PASSES, W, H, ch, depth);
    if (total != (int64_t)nfilt) { fprintf(stderr, "file %u: %lld filtered bytes planned, %u given\n", i, (long long)total, nfilt); return 3; }
    printf("%lld", (long long)total);
    for (int p = 0; p < PF_PASSES; ++p) printf(" %lld", (long long)pf_pass_offset(lace, p, W, H, ch, depth));
    bool bad = false;
    uint32_t crcs[4] = {0, 0, 0, 0};
    for (int v = 0; v < 4 && !bad; ++v) {
      const int mode = v == 1 ? ATTWARP_PNGDEC_L : v == 2 ? ATTWARP_PNGDEC_KEEP : ATTWARP_PNGDEC_RGB;
      const int oc = pf_out_channels(ctype, mode);
      const bool swap = v == 3 && oc == 3 && (ch >= 3 || ctype == 3);
      std::vector<uint32_t> ptab(256);
      for (int k = 0; k < 256; ++k) ptab[k] = pf_palette_entry(pal, k, oc, swap);
      std::vector<uint8_t> out((size_t)H * W * oc);
      std::vector<uint8_t> seen((size_t)H * W, 0);
      for (int p = 0; p < PF_PASSES && !bad; ++p) {
        const PfPass g = pf_pass(lace, p, W, H);
        if (g.w <= 0 || g.h <= 0) continue;
        const int RB = (int)pf_row_bytes(g.w, ch, depth), nu = (RB - 1) / unit;
        const uint8_t* base = filt.data() + pf_pass_offset(lace, p, W, H, ch, depth);
        std::vector<uint64_t> prev(nu, 0), cur(nu, 0);
        for (int r = 0; r < g.h && !bad; ++r) {
          const uint8_t* frow = base + (size_t)r * RB;
          const int ft = frow[0];
          if (ft > 4) { bad = true; break; }
          for (int x = 0; x < nu; ++x) {
            const uint64_t left = x ? cur[x - 1] : 0, up = prev[x], upleft = x ? prev[x - 1] : 0;
            uint64_t px = 0;
            for (int k = 0; k < unit; ++k)
              px |= (uint64_t)pd_recon(ft, frow[1 + x * unit + k], (int)((left >> (8 * k)) & 255u), (int)((up >> (8 * k)) & 255u),
                                       (int)((upleft >> (8 * k)) & 255u)) << (8 * k);
            cur[x] = px;
            const int n = std::min(ppu, g.w - x * ppu);
            for (int j = 0; j < n; ++j) {
              const uint32_t q = pf_output(ctype, pf_pixel(ctype, depth, px, j), oc, swap, ptab);
              const size_t at = (size_t)(g.y0 + r * g.dy) * W + g.x0 + (size_t)(x * ppu + j) * g.dx;
              if (seen.at(at)++) { fprintf(stderr, "file %u: pixel %zu written twice\n", i, at); return 3; }
              for (int c = 0; c < oc; ++c) out[at * oc + c] = (uint8_t)(q >> (8 * c));
            }
          }
          prev.swap(cur);
        }
      }
      if (!bad) {
        for (size_t k = 0; k < seen.size(); ++k)
          if (seen[k] != 1) { fprintf(stderr, "file %u: pixel %zu not written\n", i, k); return 3; }
        crcs[v] = crc_bytes(out.data(), (int)out.size());
      }
    }
    if (bad) printf(" filter\n");
    else printf(" %u %u %u %u\n", crcs[0], crcs[1], crcs[2], crcs[3]);
  }
  fclose(f);
  return 0;
}
