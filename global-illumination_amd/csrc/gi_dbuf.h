// gi_dbuf.h -- the one device-buffer type of the host code, and the environment knobs' reader.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#pragma GCC visibility push(hidden)
namespace gi {

// Environment knobs: tests and measurements only (every default is the measured best). All of
// them are read through env_num: GI_LOG (bit 1 device allocations >= 64 MiB, bit 2 one
// line per batch, bit 4 one line per chunk k-NN launch; stderr), GI_KNN_DBG (k-NN kernel
// diagnostics, KnnArgs::dbg), GI_DBG (render-kernel diagnostics, RenderArgs::dbg), GI_SLOT_LIMIT,
// and the exactness-tested alternatives gi_create lists (the tests select them to show that the
// default's result does not depend on them).
inline double env_num(const char *name, double def) {
  const char *s = getenv(name);
  return (s && *s) ? atof(s) : def;
}
inline int log_bits() {
  static const int bits = (int)env_num("GI_LOG", 0);
  return bits;
}
inline bool alloc_log() { return (log_bits() & 1) != 0; }

// Device buffer that only grows, owned by the object: move-only, freed by its destructor on the
// device that is current then (a function's own buffers are declared after its DeviceScope, so
// that they are freed on the right device; a context's are freed by gi_destroy / release_scratch
// with the context's device set). A growth re-allocates with 1.5x headroom: hipMalloc of tens of
// GB takes seconds on MI355X, and a frame whose batches grow a little at a time (C5's first
// render: query lists 365 M -> 431 M -> 449 M) would otherwise pay that at every step
// (the batch log showed 3.9 s and 3.2 s batches; C5 shard 1/8 cold 64.0 s vs 16.5 s warm).
struct DBuf {
  void *p = nullptr;
  size_t cap = 0;
  DBuf() = default;
  DBuf(DBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DBuf &operator=(DBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~DBuf() { release(); }
  hipError_t ensure(size_t bytes, const char *file = __builtin_FILE(), int line = __builtin_LINE()) {
    if (bytes <= cap && p) return hipSuccess;
    if (alloc_log() && bytes >= ((size_t)64 << 20)) {
      auto t0 = std::chrono::steady_clock::now();
      size_t old = cap;
      hipError_t e = grow(bytes);
      const char *base = strrchr(file, '/');
      fprintf(stderr, "[gi] alloc %.2f GB (was %.2f GB) at %s:%d: %.1f ms\n", cap / 1e9, old / 1e9,
              base ? base + 1 : file, line,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
      return e;
    }
    return grow(bytes);
  }
  hipError_t grow(size_t bytes) {
    // headroom for a buffer that has grown before: at least 1/8 above the request and at least
    // twice the old capacity. Freed device memory is cleared by the driver before it is handed
    // out again, and an allocation that finds no clean memory waits for it: C5's first frame
    // (fresh box, first process) grew its buffers in 1/8 steps to 467 GB of cumulative
    // allocation, 377 GB of it freed again, and one 32.9 GB step then waited 6.0 s (DESIGN.md
    // 3.3). Doubling (capped at 1.5x the request, so that a buffer that needs just over its old
    // capacity does not take twice that: C2's 33 GB shading list) keeps the steps few.
    size_t grown = cap ? std::max(std::min(cap * 2, bytes + bytes / 2), bytes + bytes / 8) : 0;
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
    if (grown > bytes) {  // headroom only while a quarter of the device stays free after it
      size_t fr = 0, tot = 0;
      if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < grown + tot / 4) grown = 0;
    }
    size_t want = std::max(std::max(bytes, grown), (size_t)256);
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess && want > bytes) {  // no room for the headroom: exactly what is asked
      (void)hipGetLastError();
      want = std::max(bytes, (size_t)256);
      e = hipMalloc(&p, want);
    }
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

}  // namespace gi
#pragma GCC visibility pop
