// shared batch builds (BatchShared) of the lane kernels for vMF mixtures at d = 11, 12, 13 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_vmf_wide<11, BatchShared>(GSSS_BATCH_ARGS);
template int batch_lane_vmf_wide<12, BatchShared>(GSSS_BATCH_ARGS);
template int batch_lane_vmf_wide<13, BatchShared>(GSSS_BATCH_ARGS);
}
