// GSSS_MODE_FAST launcher for a batch of vMF mixtures, and the batch builds of the lane kernels at d = 3 .. 5 (gsss_batch.h);
// the other dimensions are built in gsss_batch_vmf_{b,c,wide_a,wide_b}.hip.
#include "gsss_batch.h"

namespace gsss {

template int batch_lane_vmf<3>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_vmf<4>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_vmf<5>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);

int launch_batch_fast_vmf(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    switch (p.d) {
#define GSSS_CASE(D) \
    case D: return batch_lane_vmf<D>(p, tb, rb, bi, st);
        GSSS_BATCH_LANE_DIMS(GSSS_CASE)
#undef GSSS_CASE
#define GSSS_CASE(D) \
    case D: return batch_lane_vmf_wide<D>(p, tb, rb, bi, st);
        GSSS_BATCH_WIDE_DIMS(GSSS_CASE)
#undef GSSS_CASE
    }
    return pick_error(p);
}

}  // namespace gsss
