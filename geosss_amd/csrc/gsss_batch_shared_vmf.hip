// shared batch builds (BatchShared) of the lane kernels for vMF mixtures at d = 3 .. 5 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_vmf<3, BatchShared>(GSSS_BATCH_ARGS);
template int batch_lane_vmf<4, BatchShared>(GSSS_BATCH_ARGS);
template int batch_lane_vmf<5, BatchShared>(GSSS_BATCH_ARGS);
}
