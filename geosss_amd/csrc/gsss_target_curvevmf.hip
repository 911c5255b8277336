// Kernel instantiations for the CurveVmf target: every vector layout x {Philox, replay, numpy} draws.
#include "gsss_launch.h"

namespace gsss {
GSSS_DEFINE_TARGET_LAUNCHERS(CurveVmf)
}  // namespace gsss
