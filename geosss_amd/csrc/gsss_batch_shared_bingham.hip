// GSSS_MODE_FAST launcher for a batch of Bingham / Fisher-Bingham targets whose plan shares workgroups among targets, and the
// shared batch builds of the lane kernels at d = 3 .. 6 (gsss_batch_shared.h); the other dimensions are built in
// gsss_batch_shared_bingham_{b,wide_a,wide_b}.hip.
#include "gsss_batch_shared.h"

namespace gsss {

template int shared_lane_bingham<3>(GSSS_SHARED_ARGS);
template int shared_lane_bingham<4>(GSSS_SHARED_ARGS);
template int shared_lane_bingham<5>(GSSS_SHARED_ARGS);
template int shared_lane_bingham<6>(GSSS_SHARED_ARGS);

int launch_shared_fast_bingham(const FastPick &p, const BatchPlan &bp, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    switch (p.d) {
#define GSSS_CASE(D) \
    case D: return shared_lane_bingham<D>(p, bp, tb, rb, bi, st);
        GSSS_BATCH_LANE_DIMS(GSSS_CASE)
        GSSS_BATCH_WIDE_DIMS(GSSS_CASE)
#undef GSSS_CASE
    }
    return pick_error(p);
}

}  // namespace gsss
