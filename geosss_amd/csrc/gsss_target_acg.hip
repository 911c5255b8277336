// Kernel instantiations for the angular central Gaussian target: every vector layout x {Philox, replay, numpy} draws.
#include "gsss_launch.h"

namespace gsss {
GSSS_DEFINE_TARGET_LAUNCHERS(Acg)
}  // namespace gsss
