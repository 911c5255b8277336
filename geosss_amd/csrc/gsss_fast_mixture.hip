// GSSS_MODE_FAST dispatch for GSSS_MIXTURE targets: the lane-per-chain kernels of gsss_fast_mixture_lane.h for d = 3 .. 16
// and mixtures of at most kMixFastTerms vMF / Bingham / Fisher-Bingham / Uniform terms; everything else (a curve
// component, more terms, other d) is not built and mode "auto" runs the exact kernels.  Kernels for d = 3 .. 6 here.
#include "gsss_fast_mixture_lane.h"

namespace gsss {

template int lane_mixture<3>(const TargetBlock &, const RunBlock &, bool, FastProbe *, hipStream_t);
template int lane_mixture<4>(const TargetBlock &, const RunBlock &, bool, FastProbe *, hipStream_t);
template int lane_mixture<5>(const TargetBlock &, const RunBlock &, bool, FastProbe *, hipStream_t);
template int lane_mixture<6>(const TargetBlock &, const RunBlock &, bool, FastProbe *, hipStream_t);

int launch_fast_mixture(const TargetBlock &tb, const RunBlock &rb, bool replay, FastProbe *probe, hipStream_t st)
{
    const MixInfo mi = mix_info(tb);
    if (!mi.curve && mi.terms >= 1 && mi.terms <= kMixFastTerms) {
        switch (tb.d) {
#define GSSS_CASE(D) \
    case D: return lane_mixture<D>(tb, rb, replay, probe, st);
            GSSS_MIX_LANE_DIMS(GSSS_CASE)
#undef GSSS_CASE
        default: break;
        }
    }
    if (!probe)
        set_error("fast mode is not built for this mixture (d=%d, %d terms%s): d = 3 .. 16, at most %d vMF / Bingham terms, "
                  "no curve component", tb.d, mi.terms, mi.curve ? ", a curve component" : "", kMixFastTerms);
    return GSSS_E_UNSUPPORTED;
}

}  // namespace gsss
