// Batch builds of the exact kernels (run_kernel<.., BATCH>, gsss_device.h): vMF mixtures and Bingham targets in every vector layout,
// on the library stream.  See gsss_batch.h.
#include "gsss_batch.h"

namespace gsss {

int launch_batch_run(int vec_id, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    const bool vmf = tb.kind == GSSS_VMF_MIXTURE;
    return with_layout(vec_id, [&](auto v) {
        using V = decltype(v);
        return vmf ? do_run_batch<V, VmfMixture>(tb, rb, bi, st) : do_run_batch<V, Bingham>(tb, rb, bi, st);
    });
}

}  // namespace gsss
