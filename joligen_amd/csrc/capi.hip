// Version / error strings of the C ABI.
#include "common.h"

extern "C" int jg_version(void) { return 100; }

extern "C" const char* jg_strerror(int code) {
  switch (code) {
    case JG_OK: return "ok";
    case JG_ERR_BAD_ARG: return "bad argument (null pointer, misaligned leading dimension or unsupported shape)";
    case JG_ERR_UNSUPPORTED: return "unsupported configuration";
    case JG_ERR_LAUNCH: return "HIP launch failed";
    default: return "unknown error";
  }
}

// ---- dispatch switches --------------------------------------------------------------------------------
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace {
struct TuneDef { const char* env; int dflt; };
#define JG_TUNE_DEF(name, dflt) {"JG_" #name, dflt},
const TuneDef kTune[JG_TUNE_COUNT] = {JG_TUNE_LIST(JG_TUNE_DEF)};
#undef JG_TUNE_DEF
std::atomic<int> g_tune[JG_TUNE_COUNT];
std::once_flag g_tune_once;
void tune_init() {
  for (int i = 0; i < JG_TUNE_COUNT; ++i) {
    const char* e = getenv(kTune[i].env);
    g_tune[i].store(e ? atoi(e) : kTune[i].dflt, std::memory_order_relaxed);
  }
}
}  // namespace

namespace {
thread_local const char* g_last_kernel = "";
}
void jg_note_kernel(const char* name) { g_last_kernel = name ? name : ""; }
extern "C" const char* jg_last_kernel(void) { return g_last_kernel; }

int jg_tune(int which) {
  std::call_once(g_tune_once, tune_init);
  return g_tune[which].load(std::memory_order_relaxed);
}

extern "C" int jg_set_tuning(const char* name, int value) {
  if (!name) return JG_ERR_BAD_ARG;
  std::call_once(g_tune_once, tune_init);
  for (int i = 0; i < JG_TUNE_COUNT; ++i)
    if (!strcmp(name, kTune[i].env)) {
      g_tune[i].store(value, std::memory_order_relaxed);
      return JG_OK;
    }
  return JG_ERR_BAD_ARG;
}

extern "C" int jg_get_tuning(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < JG_TUNE_COUNT; ++i)
    if (!strcmp(name, kTune[i].env)) return jg_tune(i);
  return -1;
}
