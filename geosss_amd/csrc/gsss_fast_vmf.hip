// GSSS_MODE_FAST launcher for von Mises-Fisher mixtures: lane-per-chain kernels for d <= 16 (gsss_fast_vmf_lane.h, one
// translation unit per d), cooperative kernels beyond.  Which of them runs: gsss_fast_select.h.
#include "gsss_fast_vmf_lane.h"

namespace gsss {

int launch_fast_vmf(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, bool replay, hipStream_t st)
{
    if (p.family == kFamCoopFast) {
#define GSSS_COOP(L, S, K) \
    if (p.l == L && p.s == S && p.kc == K) return do_coopfast<CoopVec<L, S>, CoopVmf<CoopVec<L, S>, K>>(tb, rb, replay, st);
#define GSSS_COOP_K(L, S) GSSS_COOP(L, S, 3) GSSS_COOP(L, S, 5) GSSS_COOP(L, S, 10) GSSS_COOP(L, S, 16)
        GSSS_COOP_K(4, 4) GSSS_COOP_K(4, 8) GSSS_COOP_K(4, 16) GSSS_COOP_K(8, 16) GSSS_COOP_K(16, 16)
#undef GSSS_COOP_K
#undef GSSS_COOP
        return pick_error(p);
    }
    switch (p.d) {
#define GSSS_CASE(D) \
    case D: return lane_vmf<D>(p, tb, rb, replay, st);
        GSSS_VMF_LANE_DIMS(GSSS_CASE)
#undef GSSS_CASE
#define GSSS_CASE(D) \
    case D: return lane_vmf_wide<D>(p, tb, rb, st);
        GSSS_VMF_WIDE_DIMS(GSSS_CASE)
#undef GSSS_CASE
    }
    return pick_error(p);
}

}  // namespace gsss
