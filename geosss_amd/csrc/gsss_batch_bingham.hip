// GSSS_MODE_FAST dispatch for a batch of Bingham / Fisher-Bingham targets, and the batch builds of the lane kernels at
// d = 3 .. 6 (gsss_batch.h); the other dimensions are built in gsss_batch_bingham_{b,wide_a,wide_b}.hip.
#include "gsss_batch.h"

namespace gsss {

template int batch_lane_bingham<3>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);
template int batch_lane_bingham<4>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);
template int batch_lane_bingham<5>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);
template int batch_lane_bingham<6>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);

int launch_batch_fast_bingham(const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, FastProbe *probe, hipStream_t st)
{
    if (tb.d >= 3 && tb.d <= 16) {
        switch (tb.d) {
#define GSSS_CASE(D) \
    case D: return batch_lane_bingham<D>(tb, rb, bi, probe, st);
            GSSS_BATCH_LANE_DIMS(GSSS_CASE)
            GSSS_BATCH_WIDE_DIMS(GSSS_CASE)
#undef GSSS_CASE
        default: break;
        }
    }
    if (!probe)
        set_error("fast mode is not built for a batch of Bingham targets with d=%d: the batch kernels are the lane-per-chain ones "
                  "(d = 3 .. 16); use GSSS_MODE_EXACT", tb.d);
    return GSSS_E_UNSUPPORTED;
}

}  // namespace gsss
