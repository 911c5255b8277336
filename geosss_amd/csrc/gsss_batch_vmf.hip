// GSSS_MODE_FAST dispatch for a batch of vMF mixtures, and the batch builds of the lane kernels at d = 3 .. 5 (gsss_batch.h);
// the other dimensions are built in gsss_batch_vmf_{b,c,wide_a,wide_b}.hip.
#include "gsss_batch.h"

namespace gsss {

template int batch_lane_vmf<3>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);
template int batch_lane_vmf<4>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);
template int batch_lane_vmf<5>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);

int launch_batch_fast_vmf(const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, FastProbe *probe, hipStream_t st)
{
    if (tb.k >= 1 && tb.k <= 16) {
        switch (tb.d) {
#define GSSS_CASE(D) \
    case D: return batch_lane_vmf<D>(tb, rb, bi, probe, st);
            GSSS_BATCH_LANE_DIMS(GSSS_CASE)
#undef GSSS_CASE
        default: break;
        }
    }
    // d = 11 .. 16: mixtures of up to ten components, screened or all-double
    if (tb.k >= 1 && tb.k <= 10 && tb.d >= 11 && tb.d <= 16) {
        switch (tb.d) {
#define GSSS_CASE(D) \
    case D: return batch_lane_vmf_wide<D>(tb, rb, bi, probe, st);
            GSSS_BATCH_WIDE_DIMS(GSSS_CASE)
#undef GSSS_CASE
        default: break;
        }
    }
    if (!probe)
        set_error("fast mode is not built for a batch of vMF mixtures with d=%d, K=%d: the batch kernels are the lane-per-chain ones "
                  "(d = 3 .. 10 with K <= 16; d = 11 .. 16 with K <= 10); use GSSS_MODE_EXACT", tb.d, tb.k);
    return GSSS_E_UNSUPPORTED;
}

}  // namespace gsss
