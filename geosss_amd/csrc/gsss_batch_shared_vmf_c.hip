// shared batch builds (BatchShared) of the lane kernels for vMF mixtures at d = 9, 10 (see gsss_batch.h)
#include "gsss_batch.h"
namespace gsss {
template int batch_lane_vmf<9, BatchShared>(GSSS_BATCH_ARGS);
template int batch_lane_vmf<10, BatchShared>(GSSS_BATCH_ARGS);
}
