// Kernel instantiations for the angular central Gaussian target: every vector layout x {Philox, replay, numpy} draws.
#include "gsss_launch.h"

namespace gsss {
#define GSSS_RUN_CASE_Acg(ID, V, NAME) \
    case ID:                     \
        return draws == kDrawsReplay ? do_run<V, Acg, ReplayDraws>(tb, rb, st) \
               : draws == kDrawsNumpy ? do_run<V, Acg, NumpyDraws>(tb, rb, st) \
                                      : do_run<V, Acg, PhiloxDraws>(tb, rb, st);
#define GSSS_LOGPROB_CASE_Acg(ID, V, NAME) \
    case ID:                         \
        return do_logprob<V, Acg>(tb, x, n, out, grad, st);
GSSS_DEFINE_TARGET_LAUNCHERS(Acg)
}  // namespace gsss
