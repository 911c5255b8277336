// Lane-per-chain fast kernels for GSSS_MIXTURE targets of vMF and Bingham / Fisher-Bingham terms (FastMixture,
// gsss_fast.h) at d = 3 .. 16: one all-double build of kMixFastTerms terms per dimension (fewer terms run the same kernel,
// the surplus ones skipped), no single-precision screen.  The dimensions are spread over three translation units
// (compile time).
#pragma once
#include "gsss_fast.h"

namespace gsss {

template <int D>
int lane_mixture(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, bool replay, hipStream_t st)
{
    if (p.kc != kMixFastTerms) return pick_error(p);
    return do_fast<D, FastMixture<D, kMixFastTerms>>(p, tb, rb, replay, st);
}
#define GSSS_MIX_LANE_DIMS(X) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)
#define GSSS_DECLARE(D) extern template int lane_mixture<D>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
GSSS_MIX_LANE_DIMS(GSSS_DECLARE)
#undef GSSS_DECLARE

}  // namespace gsss
