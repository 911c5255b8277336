// lane-per-chain mixture kernels at d = 7 .. 11 (see gsss_fast_mixture_lane.h)
#include "gsss_fast_mixture_lane.h"
namespace gsss {
template int lane_mixture<7>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
template int lane_mixture<8>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
template int lane_mixture<9>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
template int lane_mixture<10>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
template int lane_mixture<11>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
}
