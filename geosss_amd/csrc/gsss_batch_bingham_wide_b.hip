// batch builds of the lane kernels for Bingham / Fisher-Bingham targets at d = 14, 15, 16 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_bingham<14>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_bingham<15>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
template int batch_lane_bingham<16>(const FastPick &, const TargetBlock &, const RunBlock &, const BatchInfo &, hipStream_t);
}
