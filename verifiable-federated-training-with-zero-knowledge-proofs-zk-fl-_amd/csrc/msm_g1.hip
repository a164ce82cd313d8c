// G1 instantiation of the MSM engine (separate TU: parallel build, smaller register-allocation units).
#include "msm.h"

namespace zkfl {
hipError_t zk_wtrace_bind_g1(const WtBuf& b) { return zk_wtrace_bind_tu(b); }
ZKFL_MSM_API(template, FqOps)
}  // namespace zkfl
