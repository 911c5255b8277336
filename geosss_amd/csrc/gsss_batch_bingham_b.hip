// batch builds of the lane kernels for Bingham / Fisher-Bingham targets at d = 7, 8, 9, 10 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_bingham<7>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);
template int batch_lane_bingham<8>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);
template int batch_lane_bingham<9>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);
template int batch_lane_bingham<10>(const TargetBlock &, const RunBlock &, const BatchInfo &, FastProbe *, hipStream_t);
}
