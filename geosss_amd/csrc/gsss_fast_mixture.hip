// GSSS_MODE_FAST launcher for GSSS_MIXTURE targets: the lane-per-chain kernels of gsss_fast_mixture_lane.h for d = 3 .. 16 and
// mixtures of at most kMixFastTerms vMF / Bingham / Fisher-Bingham / Uniform terms (gsss_fast_select.h); everything else (a curve
// component, more terms, other d) is not built and mode "auto" runs the exact kernels.  Kernels for d = 3 .. 6 here.
#include "gsss_fast_mixture_lane.h"

namespace gsss {

template int lane_mixture<3>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
template int lane_mixture<4>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
template int lane_mixture<5>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
template int lane_mixture<6>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);

int launch_fast_mixture(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, bool replay, hipStream_t st)
{
    switch (p.d) {
#define GSSS_CASE(D) \
    case D: return lane_mixture<D>(p, tb, rb, replay, st);
        GSSS_MIX_LANE_DIMS(GSSS_CASE)
#undef GSSS_CASE
    }
    return pick_error(p);
}

}  // namespace gsss
