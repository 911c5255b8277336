// GSSS_MODE_FAST launcher and instantiations for angular central Gaussian targets (which kernel runs: gsss_fast_select.h):
// the all-double lane kernels at d = 3 .. 10 and nothing else.
#include "gsss_fast.h"

namespace gsss {

#define GSSS_FAST_ACG_DIMS(X) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10)

int launch_fast_acg(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, bool replay, hipStream_t st)
{
    if (p.flavour != kFlavAcg) return pick_error(p);
    switch (p.d) {
#define GSSS_CASE(D) \
    case D: return do_fast<D, FastAcg<D>>(p, tb, rb, replay, st);
        GSSS_FAST_ACG_DIMS(GSSS_CASE)
#undef GSSS_CASE
    }
    return pick_error(p);
}

}  // namespace gsss
