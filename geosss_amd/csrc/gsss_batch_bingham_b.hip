// batch builds (BatchBlock) of the lane kernels for Bingham / Fisher-Bingham targets at d = 7, 8, 9, 10 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_bingham<7, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<8, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<9, BatchBlock>(GSSS_BATCH_ARGS);
template int batch_lane_bingham<10, BatchBlock>(GSSS_BATCH_ARGS);
}
