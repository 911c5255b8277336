// lane-per-chain vMF-mixture kernels at d = 9 (see gsss_fast_vmf_lane.h)
#include "gsss_fast_vmf_lane.h"
namespace gsss {
template int lane_vmf<9>(const FastPick &, const TargetBlock &, const RunBlock &, bool, hipStream_t);
}
