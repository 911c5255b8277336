// Kernel instantiations for GSSS_MIXTURE targets (Mixture, gsss_device.h): every vector layout x {Philox, replay, numpy} draws.
#include "gsss_launch.h"

namespace gsss {
GSSS_DEFINE_TARGET_LAUNCHERS(Mixture)
}  // namespace gsss
