// shared batch builds of the lane kernels for vMF mixtures at d = 6, 7, 8 (see gsss_batch_shared.h)
#include "gsss_batch_shared.h"
namespace gsss {
template int shared_lane_vmf<6>(GSSS_SHARED_ARGS);
template int shared_lane_vmf<7>(GSSS_SHARED_ARGS);
template int shared_lane_vmf<8>(GSSS_SHARED_ARGS);
}
