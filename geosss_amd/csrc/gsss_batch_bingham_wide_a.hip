// batch builds (BatchBlock) of the lane kernels for Bingham / Fisher-Bingham targets at d = 11, 12, 13 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_bingham<11, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<12, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<13, BatchBlock>(GSSS_BATCH_ARGS);
}
