// batch builds (BatchBlock) of the lane kernels for vMF mixtures at d = 14, 15, 16 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_vmf_wide<14, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_vmf_wide<15, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_vmf_wide<16, BatchBlock>(GSSS_BATCH_ARGS);
}
