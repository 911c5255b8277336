// GSSS_MODE_FAST launcher for a batch of Bingham / Fisher-Bingham targets, and the batch builds of the lane kernels at
// d = 3 .. 6 (gsss_batch.h); the other dimensions are built in gsss_batch_bingham_{b,wide_a,wide_b}.hip.
#include "gsss_batch.h"

namespace gsss {

template int batch_lane_bingham<3>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_bingham<4>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_bingham<5>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_bingham<6>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);

int launch_batch_fast_bingham(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    switch (p.d) {
#define GSSS_CASE(D) \
    case D: return batch_lane_bingham<D>(p, tb, rb, bi, st);
        GSSS_BATCH_LANE_DIMS(GSSS_CASE)
        GSSS_BATCH_WIDE_DIMS(GSSS_CASE)
#undef GSSS_CASE
    }
    return pick_error(p);
}

}  // namespace gsss
