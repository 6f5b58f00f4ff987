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

}  // namespace d3d

#define HIP_TRY(expr)                                                                                         \
  do {                                                                                                        \
    hipError_t _e = (expr);                                                                                   \
    if (_e != hipSuccess)                                                                                     \
      return d3d::fail(D3D_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
  } while (0)
