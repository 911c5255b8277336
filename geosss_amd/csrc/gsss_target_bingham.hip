// Kernel instantiations for the Bingham target: every vector layout x {Philox, replay, numpy} draws.
#include "gsss_launch.h"

namespace gsss {
GSSS_DEFINE_TARGET_LAUNCHERS(Bingham)
}  // namespace gsss
