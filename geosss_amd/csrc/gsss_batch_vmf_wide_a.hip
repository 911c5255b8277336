// batch builds of the screened lane kernels for vMF mixtures at d = 11, 12, 13 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_vmf_wide<11>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);
template int batch_lane_vmf_wide<12>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);
template int batch_lane_vmf_wide<13>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);
}
