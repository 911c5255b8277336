// batch builds of the lane kernels for Bingham / Fisher-Bingham targets at d = 7, 8, 9, 10 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_bingham<7>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_bingham<8>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_bingham<9>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_bingham<10>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
}
