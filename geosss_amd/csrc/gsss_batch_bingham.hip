// batch builds (BatchBlock) of the lane kernels for Bingham / Fisher-Bingham targets at d = 3 .. 6 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_bingham<3, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<4, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<5, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<6, BatchBlock>(GSSS_BATCH_ARGS);
}
