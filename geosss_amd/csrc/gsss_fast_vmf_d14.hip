// screened lane kernels for vMF mixtures at d = 14, one chain per lane (see gsss_fast_vmf_lane.h: lane_vmf_wide)
#include "gsss_fast_vmf_lane.h"
namespace gsss {
template int lane_vmf_wide<14>(const FastPick &, const TargetBlock &, const RunBlock &, hipStream_t);
}
