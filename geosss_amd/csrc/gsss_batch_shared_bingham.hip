// shared batch builds (BatchShared) of the lane kernels for Bingham / Fisher-Bingham targets at d = 3 .. 6 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_bingham<3, BatchShared>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<4, BatchShared>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<5, BatchShared>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<6, BatchShared>(GSSS_BATCH_ARGS);
}
