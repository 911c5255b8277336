// batch builds (BatchBlock) of the lane kernels for vMF mixtures at d = 6, 7, 8 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_vmf<6, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_vmf<7, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_vmf<8, BatchBlock>(GSSS_BATCH_ARGS);
}
