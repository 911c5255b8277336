// batch builds of the lane kernels for vMF mixtures at d = 9, 10 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_vmf<9>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_vmf<10>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
}
