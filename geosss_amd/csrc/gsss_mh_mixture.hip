// RWMH / spherical HMC kernels for GSSS_MIXTURE targets (Mixture, gsss_device.h) (gsss_mh.h), every vector layout and draw source
#include "gsss_launch.h"
#include "gsss_mh.h"

namespace gsss {
GSSS_DEFINE_MH_LAUNCHER(Mixture)
}  // namespace gsss
