// shared batch builds of the lane kernels for Bingham targets at d = 11, 12, 13 (see gsss_batch_shared.h)
#include "gsss_batch_shared.h"
namespace gsss {
template int shared_lane_bingham<11>(GSSS_SHARED_ARGS);
template int shared_lane_bingham<12>(GSSS_SHARED_ARGS);
template int shared_lane_bingham<13>(GSSS_SHARED_ARGS);
}
