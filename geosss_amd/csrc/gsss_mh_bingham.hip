// RWMH / spherical HMC kernels for the Bingham target (gsss_mh.h), every vector layout and draw source
#include "gsss_launch.h"
#include "gsss_mh.h"

namespace gsss {
GSSS_DEFINE_MH_LAUNCHER(Bingham)
}  // namespace gsss
