// Kernel instantiations for the VmfMixture target: every vector layout x {Philox, replay, numpy} draws.
#include "gsss_launch.h"

namespace gsss {
GSSS_DEFINE_TARGET_LAUNCHERS(VmfMixture)
}  // namespace gsss
