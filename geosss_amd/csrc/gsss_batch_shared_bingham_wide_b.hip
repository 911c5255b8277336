// shared batch builds of the lane kernels for Bingham targets at d = 14, 15, 16 (see gsss_batch_shared.h)
#include "gsss_batch_shared.h"
namespace gsss {
template int shared_lane_bingham<14>(GSSS_SHARED_ARGS);
template int shared_lane_bingham<15>(GSSS_SHARED_ARGS);
template int shared_lane_bingham<16>(GSSS_SHARED_ARGS);
}
