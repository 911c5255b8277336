// screened lane kernels for Bingham targets at d = 11 .. 13 (see gsss_fast_bingham_lane.h)
#include "gsss_fast_bingham_lane.h"
namespace gsss {
template int lane_bingham_wide<11>(const FastPick &, const TargetBlock &, const RunBlock &, hipStream_t);
template int lane_bingham_wide<12>(const FastPick &, const TargetBlock &, const RunBlock &, hipStream_t);
template int lane_bingham_wide<13>(const FastPick &, const TargetBlock &, const RunBlock &, hipStream_t);
}
