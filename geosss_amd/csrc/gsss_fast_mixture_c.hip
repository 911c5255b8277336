// lane-per-chain mixture kernels at d = 12 .. 16 (see gsss_fast_mixture_lane.h)
#include "gsss_fast_mixture_lane.h"
namespace gsss {
template int lane_mixture<12>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
template int lane_mixture<13>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
template int lane_mixture<14>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
template int lane_mixture<15>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
template int lane_mixture<16>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
}
