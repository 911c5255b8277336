// shared batch builds of the lane kernels for Bingham targets at d = 7 .. 10 (see gsss_batch_shared.h)
#include "gsss_batch_shared.h"
namespace gsss {
template int shared_lane_bingham<7>(GSSS_SHARED_ARGS);
template int shared_lane_bingham<8>(GSSS_SHARED_ARGS);
template int shared_lane_bingham<9>(GSSS_SHARED_ARGS);
template int shared_lane_bingham<10>(GSSS_SHARED_ARGS);
}
