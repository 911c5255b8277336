// shared batch builds (BatchShared) of the lane kernels for vMF mixtures at d = 6, 7, 8 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_vmf<6, BatchShared>(GSSS_BATCH_ARGS);
template int batch_lane_vmf<7, BatchShared>(GSSS_BATCH_ARGS);
template int batch_lane_vmf<8, BatchShared>(GSSS_BATCH_ARGS);
}
