// shared batch builds of the lane kernels for vMF mixtures at d = 9, 10 (see gsss_batch_shared.h)
#include "gsss_batch_shared.h"
namespace gsss {
template int shared_lane_vmf<9>(GSSS_SHARED_ARGS);
template int shared_lane_vmf<10>(GSSS_SHARED_ARGS);
}
