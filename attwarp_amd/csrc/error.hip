// Error reporting and version for libattwarp_hip.so.
#include "common.hpp"

#include <atomic>
#include <cstring>

namespace attwarp {

char* error_buffer() {
  static thread_local char buf[512] = {0};
  return buf;
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(error_buffer(), 512, fmt, ap);
  va_end(ap);
  return code;
}

#ifdef ATTWARP_TUNING
// stored as value + 1 so that the zero-initialised table means "automatic" everywhere
static std::atomic<int> g_tune[TUNE_COUNT];
int tune(TuneKey k) { return g_tune[k].load(std::memory_order_relaxed) - 1; }

static const char* const kTuneNames[TUNE_COUNT] = {
    "remap_variant", "remap_rows", "remap_chw_split", "remap_tiled", "remap_tile_ko", "remap_noswz", "remap_nt",
    "lanczos_variant", "clip_variant", "profiles_variant", "remap_cpw", "attn_hu", "u8_ahead", "trace_lo", "trace_hi",
    "prep_variant", "clip_ragged_variant", "pngdec_route", "jpegprog_sync_kinds", "jpegopt_given_hist", "remap_stream"};

// remap_rows.hip
int remap_rows_plan_query(int layout, int mode, int B, int C, int H, int W, int Ho, int Wo, int* packed);

#endif

}  // namespace attwarp

#ifdef ATTWARP_TUNING
extern "C" int attwarp_debug_set(const char* key, int value, int* previous) {
  using namespace attwarp;
  ATTWARP_REQUIRE(key, "debug_set: null key");
  // a query, not a key: "remap_plan:<layout>,<mode>,<B>,<C>,<H>,<W>,<H_out>,<W_out>" returns the plan the float32 staged
  // resample would take (remap_rows_plan_query) through *previous; nothing is set or launched
  if (strncmp(key, "remap_plan:", 11) == 0) {
    int a[8], packed = -1;
    ATTWARP_REQUIRE(previous && sscanf(key + 11, "%d,%d,%d,%d,%d,%d,%d,%d", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7) == 8,
                    "debug_set: remap_plan takes eight integers and a result pointer");
    for (int i = 2; i < 8; ++i) ATTWARP_REQUIRE(a[i] > 0, "debug_set: remap_plan: non-positive size");
    ATTWARP_REQUIRE(a[3] <= 4, "debug_set: remap_plan: more than 4 channels");
    const int rc = remap_rows_plan_query(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], &packed);
    *previous = packed;
    return rc;
  }
  if (strcmp(key, "reset") == 0) {
    for (auto& v : g_tune) v.store(0, std::memory_order_relaxed);
    return ATTWARP_OK;
  }
  for (int i = 0; i < TUNE_COUNT; ++i)
    if (strcmp(key, kTuneNames[i]) == 0) {
      const int old = g_tune[i].exchange(value < 0 ? 0 : value + 1, std::memory_order_relaxed);
      if (previous) *previous = old - 1;
      return ATTWARP_OK;
    }
  return fail(ATTWARP_E_ARG, "debug_set: unknown key '%s'", key);
}
#endif

extern "C" int attwarp_version(void) { return ATTWARP_VERSION; }
extern "C" const char* attwarp_last_error(void) { return attwarp::error_buffer(); }
