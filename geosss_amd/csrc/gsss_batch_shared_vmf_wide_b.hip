// shared batch builds of the lane kernels for vMF mixtures at d = 14, 15, 16 (see gsss_batch_shared.h)
#include "gsss_batch_shared.h"
namespace gsss {
template int shared_lane_vmf_wide<14>(GSSS_SHARED_ARGS);
template int shared_lane_vmf_wide<15>(GSSS_SHARED_ARGS);
template int shared_lane_vmf_wide<16>(GSSS_SHARED_ARGS);
}
