// GSSS_MODE_FAST instantiations of the group-speculative curve-vMF kernel (gsss_curvespec.h).
#include "gsss_curvespec.h"

namespace gsss {

// <L, Q, NK, +R> of the pick: the layouts select_curvespec (gsss_fast_select.h) chooses among, with the measurements behind them
int launch_curvespec(const FastPick &p, const TargetBlock &tb, const RunBlock &rb, bool replay, hipStream_t st)
{
#define GSSS_SPEC(L, Q, NK, R) \
    if (p.l == L && p.s == Q && p.kc == NK && p.r == R) return do_curvespec<L, Q, NK, R>(tb, rb, replay, st);
#define GSSS_SPEC_BOTH(L, Q) GSSS_SPEC(L, Q, 10, 0) GSSS_SPEC(L, Q, 17, 0)
    GSSS_SPEC(2, 2, 10, 0)
    GSSS_SPEC_BOTH(4, 1) GSSS_SPEC_BOTH(4, 2) GSSS_SPEC_BOTH(4, 3) GSSS_SPEC(4, 4, 10, 0)
    GSSS_SPEC(8, 3, 10, 0) GSSS_SPEC(8, 4, 10, 0)
    GSSS_SPEC_BOTH(16, 1) GSSS_SPEC_BOTH(16, 2) GSSS_SPEC_BOTH(16, 3) GSSS_SPEC_BOTH(16, 4)
    // the uneven layouts: Q quads and R tail slots per lane
    GSSS_SPEC(4, 1, 10, 1) GSSS_SPEC(4, 1, 10, 2) GSSS_SPEC(4, 2, 10, 1) GSSS_SPEC(4, 2, 10, 2) GSSS_SPEC(4, 3, 10, 1)
    GSSS_SPEC(4, 3, 10, 2) GSSS_SPEC(8, 3, 10, 1) GSSS_SPEC(8, 3, 10, 2) GSSS_SPEC(16, 3, 10, 1)
#undef GSSS_SPEC_BOTH
#undef GSSS_SPEC
    return pick_error(p);
}

}  // namespace gsss
