// shared batch builds of the lane kernels for vMF mixtures at d = 11, 12, 13 (see gsss_batch_shared.h)
#include "gsss_batch_shared.h"
namespace gsss {
template int shared_lane_vmf_wide<11>(GSSS_SHARED_ARGS);
template int shared_lane_vmf_wide<12>(GSSS_SHARED_ARGS);
template int shared_lane_vmf_wide<13>(GSSS_SHARED_ARGS);
}
