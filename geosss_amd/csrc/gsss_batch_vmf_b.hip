// batch builds of the lane kernels for vMF mixtures at d = 6, 7, 8 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_vmf<6>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_vmf<7>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_vmf<8>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
}
