// batch builds (BatchBlock) of the lane kernels for Bingham / Fisher-Bingham targets at d = 14, 15, 16 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_bingham<14, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<15, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<16, BatchBlock>(GSSS_BATCH_ARGS);
}
