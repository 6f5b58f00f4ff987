// Error reporting shared by the host translation units (engine.hip, engine_ops.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/d3d.h"
#include "d3d_kernels.h"

namespace d3d {

// stores msg as the calling thread's d3d_last_error() text (one thread-local, defined in engine.hip) and returns code
int fail(int code, const std::string& msg);

// row-kernel arguments of a plain LayerNorm over `rows` rows of width D: no positional embedding, no row classes
inline LnArgs ln_rows(int rows, int D, int rows_per_batch) {
  LnArgs a{};
  a.rows = rows; a.D = D; a.rows_per_batch = rows_per_batch; a.pos_div = 1; a.pos_mod = 1;
  return a;
}

// device memory of n elements, freed on every return path (HIP_TRY leaves early) and with its owner; reads as the pointer it holds;
// alloc / upload free first, so a re-allocation never holds both
template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }   // (move only)
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
  ~DevBuf() { reset(); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; }
  hipError_t alloc(size_t n) { reset(); const hipError_t e = hipMalloc(&p, n * sizeof(T)); if (e != hipSuccess) p = nullptr; return e; }
  hipError_t upload(const T* host, size_t n) { const hipError_t e = alloc(n); return e ? e : hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice); }
  operator T*() const { return p; }
};

}  // namespace d3d

#define HIP_TRY(expr)                                                                                         \
  do {                                                                                                        \
    hipError_t _e = (expr);                                                                                   \
    if (_e != hipSuccess)                                                                                     \
      return d3d::fail(D3D_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
  } while (0)
