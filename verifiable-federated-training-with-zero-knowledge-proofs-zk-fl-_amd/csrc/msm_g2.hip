// G2 (Fq2) instantiation of the MSM engine.
#include "msm.h"

namespace zkfl {
hipError_t zk_wtrace_bind_g2(const WtBuf& b) { return zk_wtrace_bind_tu(b); }
ZKFL_MSM_API(template, Fq2Ops)
}  // namespace zkfl
