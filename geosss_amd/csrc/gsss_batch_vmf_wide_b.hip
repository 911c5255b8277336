// batch builds of the screened lane kernels for vMF mixtures at d = 14, 15, 16 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_vmf_wide<14>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_vmf_wide<15>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_vmf_wide<16>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
}
