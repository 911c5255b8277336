// shared batch builds (BatchShared) of the lane kernels for Bingham / Fisher-Bingham targets at d = 14, 15, 16 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_bingham<14, BatchShared>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<15, BatchShared>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<16, BatchShared>(GSSS_BATCH_ARGS);
}
