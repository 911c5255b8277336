// Batch builds of the exact kernels (run_kernel<.., BATCH>, gsss_device.h): vMF mixtures and Bingham targets in every vector layout,
// on the library stream.  See gsss_batch.h.
#include "gsss_batch.h"

namespace gsss {

int launch_batch_run_vmf(int vec_id, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    switch (vec_id) {
#define GSSS_CASE(ID, V, NAME) \
    case ID: return do_run_batch<V, VmfMixture>(tb, rb, bi, st);
        GSSS_VEC_LIST(GSSS_CASE)
#undef GSSS_CASE
    }
    set_error("unknown vector layout %d", vec_id);
    return GSSS_E_INVALID;
}

int launch_batch_run_bingham(int vec_id, const TargetBlock &tb, const RunBlock &rb, const BatchInfo &bi, hipStream_t st)
{
    switch (vec_id) {
#define GSSS_CASE(ID, V, NAME) \
    case ID: return do_run_batch<V, Bingham>(tb, rb, bi, st);
        GSSS_VEC_LIST(GSSS_CASE)
#undef GSSS_CASE
    }
    set_error("unknown vector layout %d", vec_id);
    return GSSS_E_INVALID;
}

}  // namespace gsss
